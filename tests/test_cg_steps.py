"""The inputs of tests/test_cg_steps_gpu.py proved on the CPU, before a GPU is spent on them: for every f of every two-step
case, in fp64, no row's r.r after step 1 lies within a factor of 4 of the exit threshold; some row ends at step 1 and some
row does not; the fp32 oracle ends every row at the fp64 step; and the plain numpy recurrence that serves as reference
agrees with the oracle's own fp64 code."""
import numpy as np
import pytest

from tests import cg_steps_ref as ref
from tests.test_implicit_matfree_seams_gpu import CG_EXIT, _cg_rs

TWO_STEP_F = [f for f in ref.F_FUSED if len(ref.steps_for(f)) == 2]
assert min(TWO_STEP_F) == 8 and 2 in ref.F_FUSED


def test_rows_cover_the_seams():
    lens = ref.LENS
    rowptr, colidx, val = ref.rows()
    assert sorted(set(lens) - set(ref.FAST_LENS)) == sorted(set(ref.SEAM_LENS) - set(ref.FAST_LENS))
    assert set(range(34)) <= set(lens) and {63, 64, 65, 96, 97, 129, 300} <= set(lens)
    assert (np.diff(rowptr) == lens).all() and set(val) == {1.0, 2.0, 3.0, 4.0, 5.0}
    for u in range(ref.ROWS):
        c = colidx[rowptr[u]:rowptr[u + 1]]
        assert (np.diff(c) > 0).all() and (len(c) == 0 or (0 <= c[0] and c[-1] < ref.N_TABLE)), u
    for chunk in (32, 64):
        multi = lens[lens > chunk]
        assert (multi % chunk == 1).sum() >= 2 and (multi <= 2 * chunk).any() and len(multi) >= 5, chunk
    # one fast row per group: short, whole at chunk = 64 (chunked at 32), chunked at both
    a, b, c = lens[ref.FAST_ROWS]
    assert 0 < a <= 32 < b <= 64 < c
    t = ref.table(64)
    assert t.dtype == np.float32 and (t > 0).any() and (t < 0).any()


def _check_two_steps(f, A64, b64, x0, x32_1, x32_2, tag):
    _, rs1, steps = ref.reference(A64, b64, x0, 2)
    empty = np.isnan(rs1)
    assert empty.sum() == 1 and ref.LENS[empty][0] == 0
    # the window condition
    assert ref.exit_clear(rs1), (tag, rs1[(rs1 > CG_EXIT / 4) & (rs1 < CG_EXIT * 4)])
    # both sides of the exit comparison; the fast rows are the ones built to end
    ends = rs1 < CG_EXIT / 4
    assert ends[ref.FAST_ROWS].all() and (~ends & ~empty).any(), (tag, rs1[ref.FAST_ROWS])
    assert (steps[ends] == 1).all() and (steps[~ends & ~empty] == 2).all(), tag
    # the fp32 oracle ends every row where fp64 does: a row that ended keeps its one-step bits, every other row moved on
    same = (x32_1 == x32_2).all(1)
    assert same[ends].all(), (tag, np.flatnonzero(ends & ~same))
    assert not same[~ends & ~empty].any(), (tag, np.flatnonzero(~ends & ~empty & same))
    assert np.isnan(x32_1[empty]).all() and np.isnan(x32_2[empty]).all(), tag
    assert not np.isnan(x32_2[~empty]).any(), tag
    return rs1


@pytest.mark.parametrize("f", TWO_STEP_F)
def test_fused_inputs(oracle, f):
    A64, b64 = ref.systems(oracle, f)
    x0 = ref.warm_start(oracle, f)
    x64_1, x32_1, _, _ = ref.fused_refs(oracle, f, 1)
    x64_2, x32_2, _, _ = ref.fused_refs(oracle, f, 2)
    rs1 = _check_two_steps(f, A64, b64, x0, x32_1, x32_2, f"fused f={f}")
    # cg_steps is _cg_rs
    for u in (1, 17, ref.FAST_ROWS[1], ref.ROWS - 1):
        rs, k = _cg_rs(A64[u], x0[u], b64[u], 2)
        _, rs_, k_ = ref.cg_steps(A64[u], x0[u], b64[u], 2)
        assert rs == rs_ and k == k_, (f, u)
    # the numpy recurrence and the oracle's fp64 half-iteration agree to the fp32 rounding of the latter's result (half an
    # ulp: 2^-24 of the element) + 1e-11 of the scale for the order of the fp64 sums
    rowptr, colidx, val = ref.rows()
    fin = ~np.isnan(rs1)
    for iters, x64 in ((1, x64_1), (2, x64_2)):
        hi = oracle.half_iteration(rowptr, colidx, val, ref.table(f), x0.copy(), f, ref.LAM, solver="cg", cg_iters=iters,
                                   dtype=np.float64)
        assert np.isnan(hi[~fin]).all() and np.isnan(x64[~fin]).all()
        err = np.abs(hi[fin].astype(np.float64) - x64[fin])
        assert (err <= 2.0 ** -24 * np.abs(x64[fin]) + 1e-11 * np.abs(x64[fin]).max()).all(), (f, iters, err.max())


def test_one_step_only_below_f_8(oracle):
    """f = 2 (and 4): rows inside the window around the exit threshold after step 1, which is why they take one step."""
    assert ref.steps_for(2) == (1,) and ref.steps_for(8) == (1, 2)
    A64, b64 = ref.systems(oracle, 2)
    _, rs1, _ = ref.reference(A64, b64, ref.warm_start(oracle, 2), 1)
    print("f=2: rows in the window", np.flatnonzero((rs1 > CG_EXIT / 4) & (rs1 < CG_EXIT * 4)))
    x64, x32, _, _ = ref.fused_refs(oracle, 2, 1)
    assert np.isnan(x64[0]).all() and np.isnan(x32[0]).all() and not np.isnan(x32[1:]).any()


@pytest.mark.parametrize("f,half", [(f, False) for f in ref.F_SOLVE] + [(f, True) for f in ref.F_SOLVE_HALF])
def test_solve_inputs(oracle, f, half):
    A, b, x0 = ref.solve_inputs(oracle, f, half)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    x64_1, x32_1, _, _ = ref.solve_refs(oracle, f, 1, half)
    if len(ref.steps_for(f)) == 1:
        assert np.isnan(x64_1[0]).all() and not np.isnan(x64_1[1:]).any()
        return
    x64_2, x32_2, _, _ = ref.solve_refs(oracle, f, 2, half)
    rs1 = _check_two_steps(f, A64, b64, x0, x32_1, x32_2, f"solve f={f} half={half}")
    # oracle.cg in fp64 is the numpy recurrence: two fp64 evaluations, 1e-11 of the scale for the order of the sums
    fin = ~np.isnan(rs1)
    for iters, x64 in ((1, x64_1), (2, x64_2)):
        xn, _, _ = ref.reference(A64, b64, x0, iters)
        err = np.abs(xn[fin] - x64[fin])
        assert err.max() <= 1e-11 * np.abs(xn[fin]).max(), (f, half, iters, err.max())
        assert np.isnan(x64[~fin]).all()
