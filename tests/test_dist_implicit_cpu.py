"""Multi-process implicit-feedback ALS on CPU: gloo, worlds 2 and 3, one process per rank, the numpy stand-in ops of
tests/dist_implicit_helpers.py in fp64.  Both schemes of cumf_als_amd.dist_implicit must reproduce a single-process fp64
implicit ALS up to summation order (1e-9 relative), agree across ranks, keep a column without entries at exactly 0, and
report the objective of the gathered factors."""
import functools
import itertools

import numpy as np
import pytest

from tests import dist_implicit_helpers as H
from tests import implicit_ref as ref

M, N, F, LAM, ALPHA, ITERS = 120, 90, 8, 0.05, 4.0, 2
# theta_batch 1 runs the LU, theta_batch 3 the CG: every (scheme, reg, theta_batch) under both worlds
CONFIGS = [dict(scheme=s, reg=r, theta_batch=tb, solver="lu" if tb == 1 else "cg")
           for s, r, tb in itertools.product(("gather", "reduce"), ("weighted", "plain"), (1, 3))]


@functools.lru_cache(maxsize=None)
def _data():
    return H.make_data(M, N, 6000)


def _theta0():
    return (0.2 * np.random.RandomState(0).random_sample((N, F))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(reg, solver):
    return H.als_fp64(_data(), M, N, F, LAM, ALPHA, reg, solver, 3, ITERS, _theta0())


_RANKS = {}


def _ranks(world):
    """Every configuration through one spawn of `world` ranks (computed once per world, shared by the cases)."""
    cfgs = [dict(c, f=F, theta0=_theta0()) for c in CONFIGS]
    return H.run_ranks_once(_RANKS, world, world, cfgs, _data(), M, N, LAM, ALPHA, ITERS)


def test_the_data_set_has_the_columns_the_cases_need():
    from cumf_als_amd import dist as cdist

    d = _data()
    counts = np.diff(d["csc_indptr"])
    assert counts[H.EMPTY_COL] == 0 and (np.delete(counts, H.EMPTY_COL) > 0).all()
    s, e = d["csc_indptr"][H.LOCAL_COL], d["csc_indptr"][H.LOCAL_COL + 1]
    assert e - s >= 4
    for world in (2, 3):
        for solver in ("lu", "cg"):
            xb = cdist.balanced_slabs(d["csr_indptr"], world, cdist.solve_row_cost(F, solver))
            assert d["csc_indices"][s:e].max() < xb[1], (world, solver, xb)  # every entry in rank 0's slab


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", range(len(CONFIGS)), ids=lambda i: "{scheme}-{reg}-tb{theta_batch}-{solver}".format(**CONFIGS[i]))
def test_matches_single_process_fp64(world, case):
    c = CONFIGS[case]
    th_ref, x_ref = _reference(c["reg"], c["solver"])
    outs = [rank_out[case] for rank_out in _ranks(world)]
    for th, x, _ in outs:
        assert th.dtype == np.float64
        assert np.abs(th - th_ref).max() <= 1e-9 * np.abs(th_ref).max(), (world, c, np.abs(th - th_ref).max())
        assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max(), (world, c, np.abs(x - x_ref).max())
        assert (th[H.EMPTY_COL] == 0).all() and not np.signbit(th[H.EMPTY_COL]).any()
        assert np.abs(th[H.LOCAL_COL]).max() > 0
    for th, x, _ in outs[1:]:
        np.testing.assert_array_equal(th, outs[0][0])
        np.testing.assert_array_equal(x, outs[0][1])


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", range(len(CONFIGS)), ids=lambda i: "{scheme}-{reg}-tb{theta_batch}-{solver}".format(**CONFIGS[i]))
def test_loss_is_the_objective_of_the_gathered_factors(world, case):
    """The reduce scheme sums per-slab objectives: in plain mode lambda tr(Theta^T Theta) would be counted once per rank
    without its correction."""
    c, d = CONFIGS[case], _data()
    dense = H.stored_dense(d, M, N)
    for th, x, loss in (rank_out[case] for rank_out in _ranks(world)):
        sparse = ref.sparse_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], x, th, LAM, ALPHA, c["reg"])
        assert abs(loss - sparse) <= 1e-9 * abs(sparse), (world, c, loss, sparse)
        brute = ref.dense_loss(dense, x, th, LAM, ALPHA, c["reg"])
        assert abs(loss - brute) <= 1e-9 * abs(brute), (world, c, loss, brute)


def test_matfree_is_refused_on_the_reduce_theta_side():
    from cumf_als_amd import dist_implicit as di

    mat = H.host_matrix(_data(), M, N)
    for kw in (dict(solver="cg_matfree"), dict(solver="lu", solver_theta="cg_matfree")):
        with pytest.raises(ValueError, match="solver_theta"):
            di.DistImplicitALS(mat, F, LAM, ALPHA, H.NumpyImplicitOps(), scheme="reduce", **kw)
    # one rank, no process group: the X side may take it, and both schemes run without collectives
    ops = H.NumpyImplicitOps()
    ref_th, ref_x = H.als_fp64(_data(), M, N, F, LAM, ALPHA, "weighted", "cg", 3, 1, _theta0())
    for scheme in ("gather", "reduce"):
        eng = di.DistImplicitALS(mat, F, LAM, ALPHA, ops, solver="cg", solver_x="cg_matfree", scheme=scheme, theta_batch=3)
        eng.init_factors(_theta0())
        eng.iterate(1)
        assert np.abs(eng.thetaT.numpy() - ref_th).max() <= 1e-9 * np.abs(ref_th).max()
        assert np.abs(eng.full_XT().numpy() - ref_x).max() <= 1e-9 * np.abs(ref_x).max()
    with pytest.raises(ValueError):
        di.DistImplicitALS(mat, F, LAM, ALPHA, ops, scheme="scatter")
