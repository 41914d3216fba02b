"""The RMSE kernel (sse_kernel of als_common.hip, through als.sse / cumf_sse) at its seams, against tests/sse_ref.py.  Every
RMSE the project reports comes from this kernel, and the fused train SSE of every route is tested against it.

* exact: on integer inputs (ref.integer_case) the SSE is an integer that fp32 dot products and an fp64 sum deliver exactly
  in any order, so `==` is asserted -- at every f around the 16-lanes-per-rating layout (lane `sub` owns k = 2 sub,
  2 sub + 1, + 32, ...: seams at 30 / 32 / 34 and 62 / 64 / 66), f = 0 (the sum of r^2 that doALS takes), every count around
  a block (16 ratings), a wave and the grid-stride step (4096 blocks x 16 ratings), and under SURPASS_NAN (als.cu:200-215)
  with the NaN at every position around the lane seams;
* rounding: on real-valued inputs |gpu - sse64| <= ref.error_bound, which follows from the kernel's arithmetic;
* the host check of cumf_sse, the doALS path that SURPASS_NAN switches to the kernel, and ALSEngine.rmse's test grid.

tests/test_sse.py proves on the CPU that the integer cases are exact and that the bound holds for a correct evaluation."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import sse_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _args(c):
    return tuple(_dev(c[k]) for k in ("val", "row", "col", "thetaT", "XT"))


def _sse(args, count=None, surpass_nan=False, out=None):
    from cumf_als_amd import als

    out = als.sse(*args, count=count, surpass_nan=surpass_nan, out=out)
    return float(out.item())


@pytest.mark.parametrize("f", ref.F_SEAMS)
def test_exact_at_every_f_seam(alslib, f):
    m, n, count = ref.F_SEAM_SHAPE
    c = ref.integer_case(np.random.RandomState(f), m, n, f, count)
    assert {0, m - 1} <= set(c["row"]) and {0, n - 1} <= set(c["col"])
    got = _sse(_args(c))
    assert got == float(c["exact"]), (f, got, c["exact"])
    if f == 0:
        assert got == float((c["val"].astype(np.float64) ** 2).sum())


@functools.lru_cache(maxsize=None)
def _count_case():
    """The count-seam case: ratings 0 .. held - 1 of an integer case at f = 8, with one more row in each table that holds
    NaN.  prefix(count) is the device argument list in which everything past `count` is a rating of 1000 on the NaN rows."""
    m, n, f, held = ref.COUNT_SEAM_SHAPE
    c = ref.integer_case(np.random.RandomState(8), m, n, f, held)
    nan_row = np.full((1, f), np.nan, np.float32)
    c["thetaT"] = np.concatenate([c["thetaT"], nan_row])
    c["XT"] = np.concatenate([c["XT"], nan_row])
    return c, _args(c)


def _prefix(count):
    m, n, _, _ = ref.COUNT_SEAM_SHAPE
    c, (val, row, col, th, x) = _count_case()
    val, row, col = val.clone(), row.clone(), col.clone()
    val[count:], row[count:], col[count:] = 1000.0, m, n
    return c, (val, row, col, th, x)


@pytest.mark.parametrize("count", ref.COUNT_SEAMS)
def test_exact_at_every_count_seam(alslib, count):
    """A proper prefix of the arrays at every count around a block, a wave and the grid-stride step.  A read beyond `count`
    meets a rating of 1000 on NaN factor rows and shows as a wrong or NaN result."""
    c, args = _prefix(count)
    assert count < args[0].numel()
    exact = int((c["e"][:count] ** 2).sum())
    for surpass_nan in (False, True):
        got = _sse(args, count, surpass_nan)
        assert got == float(exact), (count, surpass_nan, got, exact)


def test_out_is_overwritten(alslib):
    """cumf_sse overwrites *out (hugewiki.cpp calls it on a word that holds the previous value), also when count = 0."""
    c, args = _prefix(257)
    for count in (257, 0):
        out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        assert _sse(args, count, out=out) == float(int((c["e"][:count] ** 2).sum()))


@pytest.mark.parametrize("f", ref.NAN_F)
def test_surpass_nan_exact(alslib, f):
    """SURPASS_NAN (als.cu:200-215) with the first NaN at every position around the lane seams, in the theta row, in the x
    row, and in both where the earlier one decides: the exact integer SSE of the truncated products.  Without the flag the
    result is NaN, and finite and exact again when count stops before the first touched rating."""
    c = ref.nan_case(np.random.RandomState(f), f)
    args = _args(c)
    exact = int((c["e_nan"] ** 2).sum())
    got = _sse(args, surpass_nan=True)
    assert got == float(exact), (f, got, exact)
    assert np.isnan(_sse(args, surpass_nan=False))
    # one touched rating at a time: a wrong first_nan in one variant cannot hide behind another
    for i, variant, p in c["touched"]:
        want = int((c["e_nan"][:i + 1] ** 2).sum())
        got = _sse(args, i + 1, surpass_nan=True)
        assert got == float(want), (f, i, variant, p, got, want)
    first = c["first_touched"]
    before = float(int((c["e"][:first] ** 2).sum()))
    assert _sse(args, first, surpass_nan=False) == before
    assert _sse(args, first, surpass_nan=True) == before


@functools.lru_cache(maxsize=None)
def _rounding_case(f):
    m, n, count = ref.ROUNDING_SHAPE
    c = ref.random_case(np.random.RandomState(100 + f), m, n, f, count)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    return _args(c), ref.sse64(*a, count), ref.error_bound(*a, count)


@pytest.mark.parametrize("f", ref.ROUNDING_F)
def test_rounding_within_a_priori_bound(alslib, f):
    """|gpu - sse64| <= ref.error_bound on the rounding family; the achieved fraction of the bound is printed.  Measured on
    one MI355X (profiles/sse_seams/): 3.3e-2 at f = 2, 7.7e-3 at 34, 5.4e-3 at 64, 1.2e-3 at 130, 1.3e-4 at 512 -- the bound
    adds absolute values over 4000 ratings and over the roundings of a chain, the errors carry signs.  A record, not a
    bound to tighten."""
    args, s64, bound = _rounding_case(f)
    for surpass_nan in (False, True):
        got = _sse(args, surpass_nan=surpass_nan)
        print(f"sse rounding f = {f} surpass_nan = {int(surpass_nan)}: |gpu - sse64| = {abs(got - s64):.3e}, bound {bound:.3e}, "
              f"fraction {abs(got - s64) / bound:.3e}, sse64 = {s64:.9e}")
        assert abs(got - s64) <= bound, (f, surpass_nan, got, s64, bound)


@pytest.mark.parametrize("f", ref.ROUNDING_F)
def test_run_to_run(alslib, f):
    """Two calls agree to 1e-13 relative: the order of the cross-block fp64 atomics is the only free order (250 blocks
    here), so no bit equality is claimed."""
    args, s64, _ = _rounding_case(f)
    a, b = _sse(args), _sse(args)
    assert abs(a - b) <= 1e-13 * abs(s64), (a, b)


def test_host_check_refuses(alslib, capfd):
    """cumf_sse refuses f < 0, an odd f, count < 0 and NULL arrays with something to read: hipErrorInvalidValue, one line on
    stderr that names f, no launch -- `out` keeps its prefill.  (The odd f is never launched: it would read 8 bytes at
    4-byte-aligned addresses and one float past the last table row.)  f = 0 and count = 0 stay valid."""
    from cumf_als_amd import als

    c = ref.integer_case(np.random.RandomState(1), 9, 7, 4, 40)
    val, row, col, th, x = _args(c)
    odd_th, odd_x = _dev(c["thetaT"][:, :3].copy()), _dev(c["XT"][:, :3].copy())
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    capfd.readouterr()

    def refused(call, names):
        with pytest.raises(RuntimeError, match="cumf_sse"):
            call()
        torch.cuda.synchronize()
        assert out.item() == 7.0
        err = capfd.readouterr().err
        assert err.count("\n") == 1 and err.startswith("cumf_sse:") and names in err, err

    def raw(val_, row_, col_, th_, x_, count, f):
        p = lambda t: None if t is None else t.data_ptr()
        rc = alslib.cumf_sse(p(val_), p(row_), p(col_), p(th_), p(x_), count, f, 0, out.data_ptr(), stream)
        if rc:
            raise RuntimeError(f"cumf_sse failed with HIP error {rc}")

    refused(lambda: als.sse(val, row, col, odd_th, odd_x, out=out), "f = 3")
    refused(lambda: als.sse(val, row, col, odd_th, odd_x, count=0, out=out), "f = 3")
    refused(lambda: als.sse(val, row, col, th, x, count=-1, out=out), "f = 4")
    refused(lambda: raw(val, row, col, th, x, 40, -2), "f = -2")
    refused(lambda: raw(val, row, col, th, x, 40, -1), "f = -1")
    for hole in range(5):
        a = [val, row, col, th, x]
        a[hole] = None
        refused(lambda: raw(*a, 40, 4), "f = 4")
    for hole in range(3):  # f = 0 reads no table, but still the ratings and the index arrays
        a = [val, row, col, None, None]
        a[hole] = None
        refused(lambda: raw(*a, 40, 0), "f = 0")
    # still valid: f = 0 without tables, count = 0 without anything
    raw(val, row, col, None, None, 40, 0)
    assert out.item() == float((c["val_i"] ** 2).sum())
    out.fill_(7.0)
    raw(None, None, None, None, None, 0, 4)
    assert out.item() == 0.0
    assert capfd.readouterr().err == ""


# ------------------------------------------------------------------------------------------------------------------------
# the driver: SURPASS_NAN turns the fused train RMSE of doALS off and sends both sets through the kernel
# ------------------------------------------------------------------------------------------------------------------------

M, N, F, ITERS, LAM, NNZ_TEST = 60, 50, 20, 3, 0.05, 257


@functools.lru_cache(maxsize=None)
def _driver_data():
    """60 x 50 ratings whose last two columns have no training rating -- their factors are NaN by design (a zero pivot in LU,
    test_empty_row_gives_nan_like_reference) -- and 257 test ratings of which every fourth, the first included, is on one
    of those columns.  Test rating 256, the one the reference's test grid leaves out (als.cu:1006), is a 1000."""
    from cumf_als_amd import datagen

    rng = np.random.RandomState(4)
    rows = np.concatenate([rng.randint(0, M, 1800), np.arange(M), np.arange(N - 2) % M])
    cols = np.concatenate([rng.randint(0, N - 2, 1800), np.arange(M) % (N - 2), np.arange(N - 2)])
    keep = np.unique(rows * N + cols)
    rows, cols = keep // N, keep % N
    vals = rng.randint(1, 6, len(rows)).astype(np.float32)
    t_rows = rng.randint(0, M, NNZ_TEST)
    t_cols = rng.randint(0, N - 2, NNZ_TEST)
    t_cols[0:256:4] = N - 2 + (np.arange(64) % 2)
    t_vals = rng.randint(1, 6, NNZ_TEST).astype(np.float32)
    t_vals[256] = 1000.0
    r = datagen.from_coo(M, N, rows, cols, vals, t_rows, t_cols, t_vals)
    assert r.nnz_test == NNZ_TEST and int(r.csc_indptr[N - 2]) == r.nnz  # the last two columns are empty,
    assert int(r.csr_indptr.diff().min()) > 0 and int(r.csc_indptr[:N - 1].diff().min()) > 0  # no other row or column is
    return r


def _run_driver(oracle, surpass_nan):
    from cumf_als_amd import als

    r = _driver_data()
    d = r.numpy()
    th0, x0 = oracle.init_factors(M, N, F)
    th_o, x_o = th0.copy(), x0.copy()
    _, log_o = oracle.do_als(d, th_o, x_o, M, N, F, LAM, ITERS, solver="lu", surpass_nan=surpass_nan)
    th, x, _, log = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"],
                               d["csc_data"], d["coo_row"], d["test_row"], d["test_col"], d["test_data"], M, N, F,
                               r.nnz, r.nnz_test, LAM, ITERS, 1, 1, 0, thetat_init=th0, xt_init=x0, solver="lu",
                               surpass_nan=surpass_nan, return_log=True)
    for t in (th, th_o):
        assert np.isnan(t[N - 2:]).all() and np.isfinite(t[:N - 2]).all()
    assert np.isfinite(x).all() and np.isfinite(x_o).all()
    return th, x, log.astype(np.float64), log_o


def test_doals_surpass_nan(oracle, alslib):
    """do_als(surpass_nan=True) -- the RMSE kernel for the train set too (fuse_rmse is off) -- against the oracle: finite logs
    that agree to 1e-5, the LU bound of test_sse_and_doals_rmse.  Without the flag the test RMSE is NaN in both and the
    train RMSE finite."""
    _, _, log, log_o = _run_driver(oracle, True)
    print("doALS surpass_nan logs (hip, oracle):", log.tolist(), log_o.tolist())
    assert log.shape == (ITERS, 2) and np.isfinite(log).all() and np.isfinite(log_o).all()
    assert np.abs(log - log_o).max() <= 1e-5, np.abs(log - log_o).max()
    assert (log[:, 1] < 10.0).all()  # test rating 256 (a 1000) is outside the reference's test grid
    _, _, log, log_o = _run_driver(oracle, False)
    for g in (log, log_o):
        assert np.isnan(g[:, 1]).all() and np.isfinite(g[:, 0]).all()
    assert np.abs(log[:, 0] - log_o[:, 0]).max() <= 1e-5


@pytest.mark.parametrize("nnz_test,count", [(1, 0), (256, 0), (257, 256)])
def test_engine_rmse_test_grid(oracle, alslib, nnz_test, count):
    """ALSEngine.rmse(exact_test_grid=False) covers ((nnz_test - 1) / 256) * 256 test ratings (als.cu:1006) and divides by
    nnz_test: 0, 0 and 256 of 1, 256 and 257."""
    from cumf_als_amd import als

    th, x, _, _ = _run_driver(oracle, True)
    r = _driver_data()
    cut = dataclasses.replace(r, test_row=r.test_row[:nnz_test].clone(), test_col=r.test_col[:nnz_test].clone(),
                              test_data=r.test_data[:nnz_test].clone()).to("cuda")
    eng = als.ALSEngine(cut, F, LAM, solver="lu")
    try:
        eng.init_factors(th, x)
        train, test = eng.rmse(exact_test_grid=False, surpass_nan=True)
        direct = als.sse(cut.test_data, cut.test_row, cut.test_col, eng.thetaT, eng.XT, count, True).item()
        d = cut.numpy()
        want = ref.sse64(d["test_data"], d["test_row"], d["test_col"], th, x, count, True)
        assert abs(direct - want) <= ref.error_bound(d["test_data"], d["test_row"], d["test_col"], th, x, count, True)
        assert abs(test - (direct / nnz_test) ** 0.5) <= 1e-13 * max(test, 1.0)
        if count == 0:
            assert test == 0.0 and direct == 0.0
        else:
            assert 0.0 < test < 10.0  # the 1000 of test rating 256 is not in it
        tr = (d["csr_data"], d["coo_row"], d["csr_indices"], th, x, cut.nnz, True)
        want_train = ref.sse64(*tr)
        assert abs(train ** 2 * cut.nnz - want_train) <= ref.error_bound(*tr) + 1e-12 * want_train
        assert np.isnan(eng.rmse(exact_test_grid=True, surpass_nan=False)[1])  # test rating 0 is on a NaN column
    finally:
        eng.close()
