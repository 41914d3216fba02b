"""CPU proofs behind tests/test_sse_gpu.py: the fp64 reference of the RMSE kernel (tests/sse_ref.py) against the oracle, the
a-priori error bound against a correct fp32 evaluation, and the exactness conditions of every integer case the GPU file
runs.  No GPU."""
import numpy as np
import pytest

from tests import sse_ref as ref


def _with_nan_rows(c, rng):
    """A copy of a random case with NaNs in some factor entries (a row that is NaN from k = 0, as the factors of a
    column without ratings are, and single entries)."""
    th, x = c["thetaT"].copy(), c["XT"].copy()
    th[3] = np.nan
    x[5] = np.nan
    f = th.shape[1]
    for _ in range(12):
        th[rng.randint(th.shape[0]), rng.randint(f)] = np.nan
        x[rng.randint(x.shape[0]), rng.randint(f)] = np.nan
    return dict(c, thetaT=th, XT=x)


@pytest.mark.parametrize("f", [2, 20, 34, 130])
def test_sse64_is_the_fp64_oracle(oracle, f):
    """sse64 = oracle.sse(dtype=float64) to 1e-12 relative: with and without SURPASS_NAN (als.cu:200-215), at a count below
    the array length and at count = 0."""
    rng = np.random.RandomState(f)
    m, n, nnz = 40, 30, 700
    c = ref.random_case(rng, m, n, f, nnz)
    cn = _with_nan_rows(c, rng)
    for case, surpass in ((c, False), (c, True), (cn, True)):
        a = (case["val"], case["row"], case["col"], case["thetaT"], case["XT"])
        for count in (nnz, 333, 1, 0):
            got = ref.sse64(*a, count, surpass)
            want = oracle.sse(*a, count, f, surpass_nan=surpass, dtype=np.float64)
            assert np.isfinite(want)
            assert abs(got - want) <= 1e-12 * abs(want), (f, count, surpass, got, want)
            if count == 0:
                assert got == 0.0 and want == 0.0
    # without SURPASS_NAN a NaN factor reaches the result in both
    a = (cn["val"], cn["row"], cn["col"], cn["thetaT"], cn["XT"])
    assert np.isnan(ref.sse64(*a, nnz, False)) and np.isnan(oracle.sse(*a, nnz, f, dtype=np.float64))


@pytest.mark.parametrize("f", ref.ROUNDING_F)
def test_fp32_oracle_within_error_bound(oracle, f):
    """The bound is neither vacuous nor violated by a correct fp32 evaluation: the fp32 oracle -- a serial fmaf chain, n = f
    roundings per dot product -- stays within error_bound(n = f) of sse64 on the rounding family, and the bound is a small
    fraction of the SSE itself."""
    m, n, held = ref.ROUNDING_SHAPE
    c = ref.random_case(np.random.RandomState(100 + f), m, n, f, held)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    count = 1000
    s64 = ref.sse64(*a, count)
    # The oracle also SUMS in fp32, which the bound does not describe (the kernel sums in fp64): it is called one rating at
    # a time and the squares are summed here in fp64.  What remains beyond the bound is the rounding of each square to
    # fp32, at most u e~^2 with sum e~^2 <= SSE_64 + bound.
    th, x = np.ascontiguousarray(c["thetaT"]), np.ascontiguousarray(c["XT"])
    s32 = float(sum(oracle.sse(c["val"][i:i + 1], c["row"][i:i + 1], c["col"][i:i + 1], th, x, 1, f, dtype=np.float32)
                    for i in range(count)))
    bound = ref.error_bound(*a, count, n=f)
    bound += ref.U * (s64 + bound)
    kernel_bound = ref.error_bound(*a, count)
    print(f"f = {f}: |oracle32 - sse64| = {abs(s32 - s64):.3e}, bound {bound:.3e}, kernel's bound {kernel_bound:.3e}, "
          f"sse64 {s64:.6e}")
    assert abs(s32 - s64) <= bound
    assert 0.0 < kernel_bound <= 1e-4 * s64


def test_error_bound_scales_with_roundings():
    m, n, count = ref.ROUNDING_SHAPE
    c = ref.random_case(np.random.RandomState(7), m, n, 64, count)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    assert ref.kernel_roundings(64) == 8 and ref.kernel_roundings(66) == 10 and ref.kernel_roundings(2) == 6
    assert ref.kernel_roundings(0) == 4
    assert ref.error_bound(*a, count, n=8) == ref.error_bound(*a, count) < ref.error_bound(*a, count, n=64)
    assert ref.error_bound(*a, 0) == 0.0


@pytest.mark.parametrize("f", ref.F_SEAMS)
def test_integer_case_exact_at_every_f(oracle, f):
    """integer_case asserts its magnitude conditions itself; here its "exact" is confirmed by sse64 and by BOTH oracles bit for
    bit, which is what exactness in any order means."""
    m, n, count = ref.F_SEAM_SHAPE
    c = ref.integer_case(np.random.RandomState(f), m, n, f, count)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    assert {0, m - 1} <= set(c["row"]) and {0, n - 1} <= set(c["col"])
    assert ref.sse64(*a, count) == float(c["exact"])
    assert oracle.sse(*a, count, f, dtype=np.float64) == float(c["exact"])
    if c["exact"] < 2 ** 24:  # the fp32 oracle also SUMS in fp32
        assert oracle.sse(*a, count, f, dtype=np.float32) == float(c["exact"])
    if f == 0:
        assert c["exact"] == int((c["val_i"] ** 2).sum())


def test_integer_case_exact_at_every_count():
    m, n, f, held = ref.COUNT_SEAM_SHAPE
    c = ref.integer_case(np.random.RandomState(8), m, n, f, held)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    assert max(ref.COUNT_SEAMS) < held
    for count in ref.COUNT_SEAMS:
        exact = int((c["e"][:count] ** 2).sum())
        assert exact < 2 ** 45
        assert ref.sse64(*a, count) == float(exact)


@pytest.mark.parametrize("f", ref.NAN_F)
def test_nan_case_exact(oracle, f):
    """The SURPASS_NAN case: every position occurs in all three variants, at even and odd k, the truncated errors are what
    sse64 and the fp64 oracle compute, and without SURPASS_NAN the result is NaN from the first touched rating on."""
    c = ref.nan_case(np.random.RandomState(f), f)
    a = (c["val"], c["row"], c["col"], c["thetaT"], c["XT"])
    count = len(c["val"])
    pos = {p for _, _, p in c["touched"]}
    assert pos == set(ref.nan_positions(f)) and {p % 2 for p in pos} == {0, 1}
    assert {v for _, v, _ in c["touched"]} == {"theta", "x", "both"}
    assert {int(k) % 2 for k in c["K"][[i for i, _, _ in c["touched"]]]} == {0, 1}
    exact = int((c["e_nan"] ** 2).sum())
    assert ref.sse64(*a, count, True) == float(exact)
    assert oracle.sse(*a, count, f, surpass_nan=True, dtype=np.float64) == float(exact)
    assert np.isnan(ref.sse64(*a, count, False))
    first = c["first_touched"]
    assert first == min(i for i, _, _ in c["touched"])
    assert ref.sse64(*a, first, False) == float(int((c["e"][:first] ** 2).sum()))
    assert np.isnan(ref.sse64(*a, first + 1, False))
