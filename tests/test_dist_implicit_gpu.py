"""Multi-GPU implicit-feedback ALS on the MI355X: the packed partial systems (cumf_get_hermitian_implicit_partial) and
their finish (cumf_implicit_finish) against fp64, and the engines of cumf_als_amd.dist_implicit with the HIP ops -- two
(once three) processes sharing cuda:0, collectives over gloo with host staging -- against the single-process
ImplicitALSEngine and an fp64 implicit ALS."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dist_implicit_helpers as H
from tests import implicit_ref as ref

pytestmark = pytest.mark.gpu

LAM, ALPHA = 0.05, 4.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the partial kernel ------------------------------------------------------------------

BOUNDS = {"small": [0, 50, 100, 150], "long_row": [0, 400, 800, 1200]}
HOT_COL, GAP_COL = 7, 5  # long_row: ~300 entries per slab; both sets: no entry in the first slab


@functools.lru_cache(maxsize=None)
def _ratings(kind):
    """small: 150 x 60 with 4 000 entries.  long_row: 1 200 x 60 where column HOT_COL has about 300 entries in every
    slab of 400 users (cut into chunks of 64 by the plan).  Column GAP_COL has no entry in the first slab."""
    rng = np.random.RandomState(3 if kind == "small" else 4)
    m, n = BOUNDS[kind][-1], 60
    if kind == "small":
        allowed = np.ones((m, n), bool)
        allowed[: BOUNDS[kind][1], GAP_COL] = False
        cells = rng.permutation(np.flatnonzero(allowed))[:4000]
        mask = np.zeros((m, n), bool)
        mask.flat[cells] = True
    else:
        mask = rng.random_sample((m, n)) < 0.05
        mask[:, HOT_COL] = rng.random_sample(m) < 0.75
        mask[: BOUNDS[kind][1], GAP_COL] = False
    R = np.zeros((m, n), np.float32)
    R[mask] = rng.choice(H.VALUES, int(mask.sum()))
    row, col = np.nonzero(mask)
    colT, rowT = np.nonzero(mask.T)
    return dict(m=m, n=n, csr_indptr=np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32),
                csr_indices=col.astype(np.int32), csr_data=R[row, col],
                csc_indptr=np.concatenate([[0], np.cumsum(mask.sum(0))]).astype(np.int32),
                csc_indices=rowT.astype(np.int32), csc_data=R[rowT, colT])


def _unpack(packed, f):
    iu = np.triu_indices(f)
    A = np.zeros((packed.shape[0], f, f), packed.dtype)
    A[:, iu[0], iu[1]] = packed
    A[:, iu[1], iu[0]] = packed
    return A


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("f", [8, 20, 64, 100, 128])
def test_packed_partials_of_three_slabs_sum_to_the_systems(alslib, f, reg):
    from cumf_als_amd import als
    from cumf_als_amd import dist as cdist

    pk = f * (f + 1) // 2
    for kind in ("small", "long_row"):
        d = _ratings(kind)
        m, n, bounds = d["m"], d["n"], BOUNDS[kind]
        X = (0.3 * np.random.RandomState(f).standard_normal((m, f))).astype(np.float32)
        total = np.zeros((n, pk))
        total_rhs = np.zeros((n, f))
        chunked = 0
        for g in range(3):
            x0, x1 = bounds[g], bounds[g + 1]
            rp, ci, va = cdist.slice_csr(d["csr_indptr"], d["csr_indices"], d["csr_data"], x0, x1)
            cp, ri, cv = cdist.local_csc_of_slab(rp, ci, va, n)
            rig, cvg, Xg = _dev(ri), _dev(cv), _dev(X[x0:x1])
            packed = torch.full((n, pk), float("nan"), device="cuda")
            rhs = torch.full((n, f), float("nan"), device="cuda")
            packed2, rhs2 = torch.zeros_like(packed), torch.zeros_like(rhs)
            for b in range(3):  # Theta batches as the engine cuts them: batches 2 and 3 have row_begin > 0
                off, size = b * (n // 3), n // 3 if b != 2 else n - 2 * (n // 3)
                plan = als.Plan(cp, f, off, off + size, 64 if kind == "long_row" else 0)
                chunked += plan.n_multi_rows
                for out_p, out_r in ((packed, rhs), (packed2, rhs2)):
                    als.get_hermitian_implicit_partial(plan, rig, cvg, Xg, LAM, ALPHA, reg, out_p[off:off + size],
                                                       out_r[off:off + size])
                plan.close()
            torch.cuda.synchronize()
            assert torch.equal(packed, packed2) and torch.equal(rhs, rhs2), (kind, g)  # every row written, the same bits
            p, r = packed.cpu().numpy(), rhs.cpu().numpy()
            for col in np.flatnonzero(np.diff(cp) == 0):  # rows without entries in this slab: all-zero
                assert not p[col].any() and not r[col].any(), (kind, g, col)
            if g == 0:
                assert cp[GAP_COL + 1] == cp[GAP_COL]
            if kind == "long_row":
                assert 250 <= cp[HOT_COL + 1] - cp[HOT_COL] <= 350
            total += p.astype(np.float64)
            total_rhs += r.astype(np.float64)
        assert (chunked > 0) == (kind == "long_row")  # the packed slot reduce ran
        X64 = X.astype(np.float64)
        A = _unpack(total, f) + (X64.T @ X64)[None]
        if reg == "plain":
            A += LAM * np.eye(f)
        cp, ri, cv = d["csc_indptr"], d["csc_indices"], d["csc_data"]
        A64, b64 = ref.systems(cp, ri, cv, X, LAM, ALPHA, reg)
        Aabs, _ = ref.systems(cp, ri, cv, X, LAM, ALPHA, reg, absolute=True)
        assert (np.abs(A - A64) <= 1e-5 * Aabs).all(), (kind, f, reg, np.abs(A - A64).max())
        cabs = np.zeros_like(b64)  # |b| formula: sum (1 + w) |y| over the positive entries
        for u in range(n):
            s, e = cp[u], cp[u + 1]
            c = np.where(cv[s:e] > 0, 1 + ALPHA * np.abs(cv[s:e]), 0).astype(np.float64)
            cabs[u] = c @ np.abs(X64[ri[s:e]]) if e > s else 0
        assert (np.abs(total_rhs - b64) <= 1e-5 * cabs + 1e-30).all(), (kind, f, reg, np.abs(total_rhs - b64).max())


# ---- the finish kernel -------------------------------------------------------------------

@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("f", [8, 20, 128])
def test_finish_equals_its_float32_restatement(alslib, f, reg):
    """tt = fl32(packed(min, max) + G), then + reg_add on the diagonal as a second fp32 addition (the order the header
    states); reg_add is lambda in plain mode and 0 in weighted mode."""
    from cumf_als_amd import als

    rng = np.random.RandomState(f)
    batch = 37
    packed = rng.standard_normal((batch, f * (f + 1) // 2)).astype(np.float32)
    g = rng.standard_normal((f, f)).astype(np.float32)
    G = g + g.T  # fp32 addition commutes: exactly symmetric
    reg_add = np.float32(LAM if reg == "plain" else 0.0)
    want = _unpack(packed, f) + G[None]
    assert want.dtype == np.float32
    i = np.arange(f)
    want[:, i, i] = want[:, i, i] + reg_add
    tt = als.implicit_finish(_dev(packed), _dev(G), float(reg_add))
    torch.cuda.synchronize()
    got = tt.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, got.transpose(0, 2, 1))


# ---- refusals ----------------------------------------------------------------------------

def test_out_of_scope_f_is_refused(alslib):
    from cumf_als_amd import als

    rowptr = np.array([0, 2, 3], np.int32)
    ci, va = _dev(np.array([0, 1, 1], np.int32)), _dev(np.ones(3, np.float32))
    for f in (6, 130):  # a plan of the same f exists; the entry point refuses it
        plan = als.Plan(rowptr, f)
        with pytest.raises(RuntimeError, match="cumf_get_hermitian_implicit_partial"):
            als.get_hermitian_implicit_partial(plan, ci, va, torch.zeros((2, f), device="cuda"), LAM, ALPHA)
        plan.close()
    plan = als.Plan(rowptr, 8)  # no plan has an odd f: the C entry point is asked for f = 7 directly
    buf = torch.zeros(4096, device="cuda")
    rc = alslib.cumf_get_hermitian_implicit_partial(plan._h, C.c_void_p(ci.data_ptr()), C.c_void_p(va.data_ptr()),
                                                    C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()),
                                                    C.c_void_p(buf.data_ptr()), 7, LAM, ALPHA, 0, None)
    assert rc != 0
    plan.close()
    for f in (6, 7, 130):
        packed = torch.zeros((3, f * (f + 1) // 2), device="cuda")
        with pytest.raises(RuntimeError, match="cumf_implicit_finish"):
            als.implicit_finish(packed, torch.zeros((f, f), device="cuda"), LAM)


def test_matfree_is_refused_on_the_reduce_theta_side(alslib):
    from cumf_als_amd import dist_implicit as di

    mat = H.host_matrix(H.make_data(), 120, 90)
    ops = di.HipImplicitOps("cuda")
    for kw in (dict(solver="cg_matfree"), dict(solver="lu", solver_theta="cg_matfree")):
        with pytest.raises(ValueError, match="solver_theta"):
            di.DistImplicitALS(mat, 20, LAM, ALPHA, ops, scheme="reduce", **kw)
    with pytest.raises(ValueError, match="128"):  # the materialising solvers stop at f = 128 under both schemes
        di.DistImplicitALS(mat, 130, LAM, ALPHA, ops, solver="lu", scheme="gather")


# ---- the engines -------------------------------------------------------------------------

M, N, ITERS = 120, 90, 2
# (scheme, solver, f, reg): both schemes x both solvers x f = 20 (weighted) and 32 (plain); the matrix-free CG under `gather`
WORLD2 = [(s, v, f, "weighted" if f == 20 else "plain") for f in (20, 32) for s in ("gather", "reduce") for v in ("lu", "cg")]
WORLD2.append(("gather", "cg_matfree", 20, "weighted"))
WORLD3 = [("reduce", "lu", 20, "weighted")]
TOL = {"lu": 2e-4, "cg": 3e-3, "cg_matfree": 3e-3}  # the bounds of tests/test_dist_gpu.py


def _theta0(f):
    return (0.2 * np.random.RandomState(0).random_sample((N, f))).astype(np.float32)


def _device_ratings(d, m, n):
    from cumf_als_amd import datagen

    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(d["csr_indptr"]))
    one = torch.zeros(1, dtype=torch.int32, device="cuda")
    return datagen.Ratings(m=m, n=n, coo_row=torch.from_numpy(rows).cuda(), test_row=one, test_col=one.clone(),
                           test_data=torch.zeros(1, device="cuda"), **t)


@functools.lru_cache(maxsize=None)
def _single_process(solver, f, reg):
    """(thetaT, XT) of the single-process ImplicitALSEngine from the same initial factors."""
    from cumf_als_amd import als

    e = als.ImplicitALSEngine(_device_ratings(H.make_data(M, N, 6000), M, N), f, LAM, ALPHA, solver=solver, cg_iters=3,
                              reg=reg)
    e.init_factors(_theta0(f))
    e.iterate(ITERS)
    torch.cuda.synchronize()
    out = e.thetaT.cpu().numpy().copy(), e.XT.cpu().numpy().copy()
    e.close()
    return out


_RANKS = {}


def _ranks(world):
    """Every case of one world through ONE spawn of `world` processes sharing cuda:0 (with the parent at most 4 processes
    hold the GPU), computed once and shared by the cases."""
    cases = WORLD2 if world == 2 else WORLD3
    cfgs = [dict(scheme=s, solver=v, f=f, reg=r, theta_batch=2, theta0=_theta0(f)) for s, v, f, r in cases]
    return H.run_ranks_once(_RANKS, world, world, cfgs, H.make_data(M, N, 6000), M, N, LAM, ALPHA, ITERS, ops_kind="hip",
                            timeout=300)


def _check_engine_case(world, cases, i):
    scheme, solver, f, reg = cases[i]
    th_ref, x_ref = _single_process(solver, f, reg)
    outs = [rank_out[i] for rank_out in _ranks(world)]
    d = H.make_data(M, N, 6000)
    for th, x, loss in outs:
        dth, dx = np.abs(th - th_ref).max(), np.abs(x - x_ref).max()
        print(f"world {world} {scheme} {solver} f={f} {reg}: max|dTheta| {dth:.3e} (scale {np.abs(th_ref).max():.3f}) "
              f"max|dX| {dx:.3e} (scale {np.abs(x_ref).max():.3f})")
        assert dth <= TOL[solver] * np.abs(th_ref).max()
        assert dx <= TOL[solver] * np.abs(x_ref).max()
        assert (th[H.EMPTY_COL] == 0).all()
        want = ref.sparse_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], x, th, LAM, ALPHA, reg)
        assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    for th, x, _ in outs[1:]:  # tables equal across ranks, bit for bit
        np.testing.assert_array_equal(th, outs[0][0])
        np.testing.assert_array_equal(x, outs[0][1])
    if solver == "lu":  # no further from the fp64 ALS than twice the single-process engine's own distance
        th64, x64 = H.als_fp64(d, M, N, f, LAM, ALPHA, reg, "lu", 3, ITERS, _theta0(f))
        for got, single, exact in ((outs[0][0], th_ref, th64), (outs[0][1], x_ref, x64)):
            e_d, e_s = np.abs(got - exact).max(), np.abs(single - exact).max()
            print(f"   distance from the fp64 ALS: distributed {e_d:.3e}, single-process {e_s:.3e}")
            assert e_d <= 2 * e_s + 1e-5 * np.abs(exact).max()


@pytest.mark.parametrize("case", range(len(WORLD2)), ids=lambda i: "{}-{}-f{}-{}".format(*WORLD2[i]))
def test_world2_hip_matches_single_process(alslib, case):
    _check_engine_case(2, WORLD2, case)


@pytest.mark.parametrize("case", range(len(WORLD3)), ids=lambda i: "{}-{}-f{}-{}".format(*WORLD3[i]))
def test_world3_hip_matches_single_process(alslib, case):
    _check_engine_case(3, WORLD3, case)


# ---- the reduce path on one rank ---------------------------------------------------------

@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_local_slab_reduce_single_rank(alslib, solver):
    """`DistImplicitALS.from_local_slab` with one rank and no process group (slab-local CSC built on the device, packed
    partials -> finish -> solve per Theta batch) == the single-process engine."""
    from cumf_als_amd import dist_implicit as di

    f, reg = 20, "weighted"
    r = _device_ratings(H.make_data(M, N, 6000), M, N)
    th_ref, x_ref = _single_process(solver, f, reg)
    eng = di.DistImplicitALS.from_local_slab(M, N, [0, M], r.csr_indptr, r.csr_indices, r.csr_data, f, LAM, ALPHA,
                                             di.HipImplicitOps("cuda"), solver=solver, cg_iters=3, reg=reg, theta_batch=3)
    eng.init_factors(_theta0(f))
    eng.iterate(ITERS)
    torch.cuda.synchronize()
    th, x = eng.thetaT.cpu().numpy(), eng.full_XT().cpu().numpy()
    eng.close()
    assert np.abs(th - th_ref).max() <= TOL[solver] * np.abs(th_ref).max()
    assert np.abs(x - x_ref).max() <= TOL[solver] * np.abs(x_ref).max()
    assert (th[H.EMPTY_COL] == 0).all()


def test_local_slab_reduce_loss_is_non_increasing(alslib):
    from cumf_als_amd import dist_implicit as di

    f = 20
    r = _device_ratings(H.make_data(M, N, 6000), M, N)
    eng = di.DistImplicitALS.from_local_slab(M, N, [0, M], r.csr_indptr, r.csr_indices, r.csr_data, f, LAM, ALPHA,
                                             di.HipImplicitOps("cuda"), solver="lu", theta_batch=3)
    eng.init_factors(_theta0(f))
    eng.update_x()
    prev = eng.loss()
    losses = [prev]
    for _ in range(3):
        for half in (eng.update_theta, eng.update_x):
            half()
            cur = eng.loss()
            losses.append(cur)
            assert cur <= prev + 1e-6 * abs(prev), losses  # the slack of tests/test_implicit_gpu.py
            prev = cur
    eng.close()
    print(f"reduce scheme, one rank, lu: losses {losses}")
