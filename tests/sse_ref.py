"""Plain numpy reference of the RMSE kernel (sse_kernel of als_common.hip, reached through cumf_sse / als.sse), shared by
tests/test_sse.py (CPU) and tests/test_sse_gpu.py (GPU).

* `sse64`: the reference program's RMSE kernel (als.cu:191-219; the dot product and its SURPASS_NAN break are als.cu:200-215)
  evaluated in fp64 over the first `count` ratings.
* `error_bound`: the a-priori bound on |SSE_gpu - SSE_64| that follows from the kernel's arithmetic -- nothing in it is
  measured.
* `integer_case`: inputs on which the SSE is an integer that fp32 and fp64 evaluate exactly in ANY summation order, so
  that the kernel must return it bit for bit.
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


def _rows(row, col, thetaT, XT, count):
    th = np.asarray(thetaT)[np.asarray(col[:count], np.int64)].astype(np.float64)
    x = np.asarray(XT)[np.asarray(row[:count], np.int64)].astype(np.float64)
    return th, x


def products(row, col, thetaT, XT, count, surpass_nan=False):
    """theta[col, k] * x[row, k] in fp64, count x f; with surpass_nan the products from the first k at which either
    factor is NaN are dropped (als.cu:206-207: the break)."""
    th, x = _rows(row, col, thetaT, XT, count)
    p = th * x
    if surpass_nan:
        nan = np.isnan(th) | np.isnan(x)
        p = np.where(np.cumsum(nan, axis=1) == 0, p, 0.0)
    return p


def errors64(val, row, col, thetaT, XT, count, surpass_nan=False):
    """e_i = val_i - sum_{k < K} theta[col_i, k] x[row_i, k] in fp64 (als.cu:198-215)."""
    p = products(row, col, thetaT, XT, count, surpass_nan)
    return np.asarray(val[:count], np.float64) - p.sum(axis=1)


def sse64(val, row, col, thetaT, XT, count, surpass_nan=False):
    """Sum of e_i^2 over the first `count` ratings in fp64 (als.cu:216 + the Sasum of als.cu:988)."""
    e = errors64(val, row, col, thetaT, XT, count, surpass_nan)
    return float(np.sum(e * e))


def kernel_roundings(f):
    """Roundings on the way to one rating's dot product in sse_kernel: lane `sub` of the rating's 16 owns k = 2 sub,
    2 sub + 1, + 32, ... -- at most 2 ceil(f / 32) fmaf in its chain -- and four butterfly additions join the lanes."""
    return 2 * ((f + 31) // 32) + 4


def error_bound(val, row, col, thetaT, XT, count, surpass_nan=False, n=None):
    """A-priori bound on |SSE_fp32 - SSE_64| of an fp32 evaluation whose dot product sees at most `n` roundings (default:
    sse_kernel's, `kernel_roundings`; a serial chain over k has n = f) and whose squares are summed in fp64.

    With u = 2^-24 and gamma = n u / (1 - n u) the computed dot product is within gamma sum_k |theta_k x_k| of the exact
    one (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the subtraction from the rating adds one
    rounding of the computed error, so per rating
        delta_i = gamma sum_k |theta_k x_k| + u (|e_i| + gamma sum_k |theta_k x_k|)
    and |e~_i^2 - e_i^2| <= 2 |e_i| delta_i + delta_i^2.  The squares and their sum are fp64 (the products of two fp32
    values are exact there); 1e-12 SSE_64 covers that accumulation and the order of the cross-block atomics."""
    f = np.asarray(thetaT).shape[-1]
    if n is None:
        n = kernel_roundings(f)
    gamma = n * U / (1.0 - n * U)
    p = products(row, col, thetaT, XT, count, surpass_nan)
    e = np.abs(np.asarray(val[:count], np.float64) - p.sum(axis=1))
    s_abs = np.abs(p).sum(axis=1)
    delta = gamma * s_abs + U * (e + gamma * s_abs)
    return float(np.sum(2.0 * e * delta + delta * delta) + 1e-12 * np.sum(e * e))


def integer_case(rng, m, n, f, count):
    """Factors that are integers in [-4, 4] stored as fp32 (thetaT n x f, XT m x f), ratings that are integers 1..5, `count`
    (row, col) pairs of which the first two are (0, 0) and (m - 1, n - 1): the first and the last row of both tables.

    Then every product and every partial sum of a dot product is an integer of magnitude <= 16 f <= 8192 < 2^24, every
    e an integer with e^2 < 2^27 and sum e^2 < 2^45 for count <= 2^18: each operation of an fp32 dot product and of an
    fp64 sum of squares is exact in whatever order it runs, and the SSE is the int64 value returned as "exact" ("e": the
    int64 error of each rating, for the SSE of a prefix).  The conditions are asserted here on the data."""
    assert 0 <= f and 16 * f <= 8192 and 0 <= count <= 2 ** 18
    th_i = rng.randint(-4, 5, size=(n, f)).astype(np.int64)
    x_i = rng.randint(-4, 5, size=(m, f)).astype(np.int64)
    row = rng.randint(0, m, size=count).astype(np.int32)
    col = rng.randint(0, n, size=count).astype(np.int32)
    row[:2] = [0, m - 1][:count]
    col[:2] = [0, n - 1][:count]
    val_i = rng.randint(1, 6, size=count).astype(np.int64)
    p = th_i[col] * x_i[row]
    assert np.abs(p).sum(axis=1).max(initial=0) < 2 ** 24          # every partial sum, in any order
    e = val_i - p.sum(axis=1)
    assert (e * e).max(initial=0) < 2 ** 27 and int((e * e).sum()) < 2 ** 45
    thetaT, XT, val = th_i.astype(np.float32), x_i.astype(np.float32), val_i.astype(np.float32)
    assert (thetaT.astype(np.int64) == th_i).all() and (XT.astype(np.int64) == x_i).all()
    return {"val": val, "row": row, "col": col, "thetaT": thetaT, "XT": XT, "th_i": th_i, "x_i": x_i, "val_i": val_i,
            "e": e, "exact": int((e * e).sum())}


def random_case(rng, m, n, f, count):
    """The rounding family: factors 0.3 N(0, 1), ratings an integer 1..5 plus the planted model theta . x rounded to fp32, so
    that e stays of order 1 while sum_k |theta_k x_k| grows with f; the first two ratings touch the first and the last
    row of both tables."""
    thetaT = (0.3 * rng.standard_normal((n, f))).astype(np.float32)
    XT = (0.3 * rng.standard_normal((m, f))).astype(np.float32)
    row = rng.randint(0, m, size=count).astype(np.int32)
    col = rng.randint(0, n, size=count).astype(np.int32)
    row[:2], col[:2] = [0, m - 1], [0, n - 1]
    model = (thetaT[col].astype(np.float64) * XT[row].astype(np.float64)).sum(axis=1)
    val = (rng.randint(1, 6, size=count) + model).astype(np.float32)
    return {"val": val, "row": row, "col": col, "thetaT": thetaT, "XT": XT}


# what tests/test_sse_gpu.py runs, so that tests/test_sse.py can prove the exactness conditions of every case on the CPU
F_SEAMS = (0, 2, 4, 30, 32, 34, 62, 64, 66, 100, 126, 128, 130, 206, 256, 512)
F_SEAM_SHAPE = (37, 53, 1000)                                    # m, n, ratings
COUNT_SEAMS = (0, 1, 15, 16, 17, 255, 256, 257, 65535, 65536, 65537, 65536 + 4095 * 16 + 1, 131073)
COUNT_SEAM_SHAPE = (37, 53, 8, 131100)                           # m, n, f, ratings held
NAN_F = (2, 34, 66)
NAN_SHAPE = (64, 64, 160)                                        # m, n, ratings
ROUNDING_F = (2, 34, 64, 130, 512)
ROUNDING_SHAPE = (300, 200, 4000)                                # m, n, ratings


def nan_positions(f):
    return sorted({p for p in (0, 1, 2, 31, 32, 33, f - 2, f - 1) if 0 <= p < f})


def nan_case(rng, f):
    """The SURPASS_NAN case at f: an integer case of NAN_SHAPE whose ordinary ratings use table rows 0..31 only, and, for
    every position p of nan_positions(f), three touched ratings -- a NaN at theta[p], a NaN at x[p], and NaNs at
    theta[p] and x[q] with q != p, where the earlier one decides -- each with a theta row and an x row of its own
    (32 + j for the j-th touched rating) and two untouched ratings between it and the next.  The first touched rating is
    rating 40.  Returns the case with the NaNs planted, "K" (the number of products each rating keeps) and "e_nan": the
    int64 error of every rating under SURPASS_NAN."""
    m, n, count = NAN_SHAPE
    c = integer_case(rng, m, n, f, count)
    c["row"][2:] = rng.randint(0, 32, size=count - 2)
    c["col"][2:] = rng.randint(0, 32, size=count - 2)
    c["row"][1], c["col"][1] = 31, 31
    K = np.full(count, f, np.int64)
    touched = []
    for p in nan_positions(f):
        q = (p + 3) % f if f > 2 else 1 - p
        for variant in ("theta", "x", "both"):
            j = len(touched)
            i = 40 + 3 * j
            assert 32 + j < min(m, n) and i < count
            c["row"][i], c["col"][i] = 32 + j, 32 + j
            if variant in ("theta", "both"):
                c["thetaT"][32 + j, p] = np.nan
            if variant == "x":
                c["XT"][32 + j, p] = np.nan
            if variant == "both":
                c["XT"][32 + j, q] = np.nan
            K[i] = min(p, q) if variant == "both" else p
            touched.append((i, variant, p))
    keep = np.arange(f)[None, :] < K[:, None]
    prod = c["th_i"][c["col"]] * c["x_i"][c["row"]]
    c["e_nan"] = c["val_i"] - np.where(keep, prod, 0).sum(axis=1)
    e_plain = c["val_i"] - prod.sum(axis=1)
    assert (c["e_nan"] ** 2).max() < 2 ** 27 and (e_plain ** 2).max() < 2 ** 27
    c["K"], c["touched"], c["first_touched"] = K, touched, 40
    c["e"] = e_plain  # valid for the untouched ratings: the SSE of a prefix that stops before the first touched one
    return c
