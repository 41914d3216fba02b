"""The materialising API (Gram batch -> batched solver -> quadratic terms) at the f values where its implementation changes.

  * cumf_lu_solve_batched: register / LDS solvers up to f = 200, lu_global_kernel (als_generic.hip) above.  The tile kernels,
    and with them cumf_get_hermitian_packed and the `reduce` scheme, reach f = 207: f = 201 .. 207 is materialised by the tile
    kernels and solved by the kernel of the range above them.
  * cumf_cg_solve_batched: LDS-resident up to f = 128, cg_global_kernel above; the fp16 entry ends at f = 256.
  * cumf_quadratic_sse_terms ends at f = 256.

include/cumf_als_capi.h promises that the solvers leave A and b as they were, and the `reduce` scheme relies on it: its train
SSE is the quadratic form of the batch it has just solved (dist.py, als_dist.cpp).  Every test here therefore checks the inputs
bit for bit after the call, besides the result.

One set of systems serves every case: the item side of a 400 x 40 rating matrix (about 300 ratings per item, more than
features at every f up to 207) + one item of 3 ratings + one item without ratings -- 42 systems.  Tolerances are the
project's own for the same quantities (test_gpu_parity.py, test_dist_gpu.py): 2e-5 max|x| for the register LU, bit equality for
the oracle-order LU, 1e-4 ||b|| (fp16 storage: 2e-3 ||b||) on the CG residual, 2e-6 sum |q| for the quadratic terms, 2e-5 for the
train-SSE identity.  That identity is only meaningful while the SSE is a visible part of sum r^2 (below ~1e-3 it is cancellation
noise: DistALS._trusted_sse); the tests that use it assert SSE >= 1e-2 sum r^2 in fp64, which ratings and lambda were chosen to
satisfy on the CPU oracle (0.12 for the chain, 0.07 for DistALS at lambda = 0.2).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LAM = 0.05
USERS, ITEMS = 400, 40
LU_F = [200, 201, 202, 206, 207, 208]
CG_F = [128, 130, 202, 206]
# The item of 3 ratings: its users and ratings.
SHORT_USERS, SHORT_RATINGS = (19, 32, 53), (5.0, 1.0, 2.0)

_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _factors(rows, f, seed):
    rng = np.random.RandomState(seed)
    return (0.2 * rng.random_sample((rows, f))).astype(np.float32)


def _item_side():
    """(row pointer, user ids, ratings) of the 42 systems: the CSC of a 400 x 40 set with uniform degrees, then an item of 3
    ratings and an item of none."""
    if "set" not in _cache:
        from cumf_als_amd import datagen

        d = datagen.synth_ratings(USERS, ITEMS, 12000, 200, seed=31, row_alpha=0.0, col_alpha=0.0).numpy()
        ptr = d["csc_indptr"].astype(np.int64)
        ptr = np.concatenate([ptr, [ptr[-1] + 3, ptr[-1] + 3]])
        idx = np.concatenate([d["csc_indices"].astype(np.int32), np.array(SHORT_USERS, np.int32)])
        val = np.concatenate([d["csc_data"].astype(np.float32), np.array(SHORT_RATINGS, np.float32)])
        lens = np.diff(ptr)
        assert len(lens) == 42 and lens[-1] == 0 and lens[-2] == 3 and lens[:-2].min() > 207
        _cache["set"] = _frozen(ptr, idx, val)
    return _cache["set"]


def _systems(oracle, f):
    """The oracle's fp32 systems of the set at f (one fmaf chain per entry) on the table `_factors(USERS, f, 1)`, built once per
    f and read-only: (A, b, keep) with keep = the systems that have ratings."""
    if ("sys", f) not in _cache:
        ptr, idx, val = _item_side()
        A, b = oracle.gram_rhs(ptr, idx, val, _factors(USERS, f, 1), f, LAM)
        _cache["sys", f] = _frozen(A, b, np.diff(ptr) > 0)
    return _cache["sys", f]


def _bits(t):
    """A device tensor as its bit pattern on the host (NaN compares equal to itself)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).cpu().numpy()


def _same_bits(t, before):
    return np.array_equal(_bits(t), before)


@pytest.mark.parametrize("f,exact", [(f, False) for f in LU_F] + [(206, True)])
def test_lu_solve_leaves_its_inputs_intact(oracle, alslib, monkeypatch, f, exact):
    """als.lu_solve on both sides of f = 200: A and b on the device keep their bits, a second solve on the same tensors returns
    the same bits, and the solution is the oracle's -- to 2e-5 max|x| from the register LU (f <= 200, as test_lu_solve), bit for
    bit from lu_global_kernel (f > 200, the claim test_generic_gram_and_lu_above_the_tile_range_are_bit_exact makes for it at
    f >= 210).  The system without ratings is 0 / 0: NaN in the oracle, never a finite answer from the library.

    CUMF_ALS_LU_EXACT=1 at f = 206: cumf_lu_solve_batched decides on f > 200 before it reads the switch, so the call runs
    lu_global_kernel like the default does -- it solves, bit-equal to the oracle, and the LDS solver of the switch (whose f x
    (f + 1) system would need 170 KB of LDS at f = 206, more than the 160 KB a workgroup has) is never asked."""
    _need_gpu()
    from cumf_als_amd import als

    A, b, keep = _systems(oracle, f)
    x_o = oracle.lu(A, b, f)
    assert np.isnan(x_o[~keep]).all()
    if exact:
        monkeypatch.setenv("CUMF_ALS_LU_EXACT", "1")
    Ag, bg = torch.from_numpy(A.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    a_bits, b_bits = _bits(Ag), _bits(bg)
    x1 = als.lu_solve(Ag, bg)
    torch.cuda.synchronize()
    a_kept, b_kept = _same_bits(Ag, a_bits), _same_bits(bg, b_bits)
    x2 = als.lu_solve(Ag, bg)
    torch.cuda.synchronize()
    x1, x2 = x1.cpu().numpy(), x2.cpu().numpy()
    err = np.abs(x1[keep] - x_o[keep]).max()
    print(f"lu_solve f={f} exact={exact}: A intact {a_kept}, b intact {b_kept}, second solve equal "
          f"{np.array_equal(x1, x2, equal_nan=True)}, max|x - x_o| = {err:.3e} (max|x_o| = {np.abs(x_o[keep]).max():.3e})")
    assert a_kept, "cumf_lu_solve_batched modified A"
    assert b_kept, "cumf_lu_solve_batched modified b"
    np.testing.assert_array_equal(x2, x1)
    assert _same_bits(Ag, a_bits) and _same_bits(bg, b_bits)
    if f > 200:
        np.testing.assert_array_equal(x1[keep], x_o[keep])
        assert np.isnan(x1[~keep]).all()
    else:
        assert err <= 2e-5 * np.abs(x_o[keep]).max(), err
        assert not np.isfinite(x1[~keep]).any()


def _residuals(A, b, x):
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    return np.linalg.norm(np.einsum("bij,bj->bi", A64, x.astype(np.float64)) - b64, axis=1), np.linalg.norm(b64, axis=1)


def _cg_warm_start(batch, f):
    """The warm start of test_cg_solve, except for the item of 3 ratings.  Its system is 0.15 I + a rank-3 matrix; from a
    generic start CG ends it in four steps, and the squared residual before the last one is set by the start's component
    outside the three factor rows: (0.15 |x0_perp|)^2 ~ 1e-4 at every f used here, which is the solver's exit threshold
    (rsnew < 1e-4, cg.cu:128).  At that discontinuity two correct fp32 recurrences may leave by different exits -- the
    oracle's own fp32 and fp64 runs do for some draws of the three users, and then end 2.3e-4 ||b|| apart, more than the
    1e-4 ||b|| allowed here.  So this one start lies in the span of the item's factor rows: three steps, the squared residuals
    before the last at least a decade above the threshold and the last ten decades below (fp64 recurrence on the oracle's
    systems, all six cases), and the oracle's fp32 and fp64 iterates within 2.4e-5 ||b|| of each other on every system."""
    x0 = _factors(batch, f, 9) * 0.1
    x0[-2] = 0.1 * _factors(USERS, f, 1)[list(SHORT_USERS)].mean(0)
    return x0.astype(np.float32)


@pytest.mark.parametrize("f,half", [(f, False) for f in CG_F] + [(130, True), (256, True)])
def test_cg_solve_leaves_its_inputs_intact(oracle, alslib, f, half):
    """als.cg_solve (6 iterations, warm-started: _cg_warm_start) on both sides of f = 128 -- the LDS-resident CG against
    cg_global_kernel -- and in the gap above the LU's seam: A and b keep their bits; the iterate is as good a solution as the
    oracle's, ||A x - b|| within 1e-4 ||b|| of the oracle's residual per system (the rule of test_cg_solve).  With fp16 storage
    of A (f = 130, and f = 256, the last f of that entry): against the oracle's CG on the widened halves, 2e-3 ||b|| (the
    bound of test_fp16_gram_storage)."""
    _need_gpu()
    from cumf_als_amd import als

    A, b, keep = _systems(oracle, f)
    x0 = _cg_warm_start(len(b), f)
    if half:
        A = A.astype(np.float16)  # round to nearest even, as Tensor.half() does
        Ag = torch.from_numpy(A.copy()).cuda()
        assert Ag.dtype == torch.float16
        A = A.astype(np.float32)
    else:
        Ag = torch.from_numpy(A.copy()).cuda()
    x_o = oracle.cg(A, x0, b, f, 6)
    bg = torch.from_numpy(b.copy()).cuda()
    a_bits, b_bits = _bits(Ag), _bits(bg)
    x = als.cg_solve(Ag, torch.from_numpy(x0.copy()).cuda(), bg, 6)
    torch.cuda.synchronize()
    assert _same_bits(Ag, a_bits), "the batched CG modified A"
    assert _same_bits(bg, b_bits), "the batched CG modified b"
    x = x.cpu().numpy()
    assert np.isfinite(x[keep]).all()
    res_h, nb = _residuals(A, b, x)
    res_o, _ = _residuals(A, b, x_o)
    gap = (np.abs(res_h - res_o) / np.where(keep, nb, 1.0))[keep]
    print(f"cg_solve f={f} half={half}: max |res_hip - res_oracle| / ||b|| = {gap.max():.3e}, "
          f"max res_oracle / ||b|| = {(res_o[keep] / nb[keep]).max():.3e}")
    assert (gap <= (2e-3 if half else 1e-4)).all(), gap.max()


def test_cg_fp16_refuses_f_above_256(alslib):
    """cumf_cg_solve_batched_fp16 ends at f = 256: f = 258 is refused before anything is launched."""
    _need_gpu()
    from cumf_als_amd import als

    f = 258
    A = torch.zeros((2, f, f), dtype=torch.float16, device="cuda")
    b = torch.ones((2, f), device="cuda")
    x = torch.zeros((2, f), device="cuda")
    with pytest.raises(RuntimeError, match="cumf_cg_solve_batched_fp16"):
        als.cg_solve(A, x, b, 6)
    torch.cuda.synchronize()
    assert not x.any()


def test_quadratic_terms_up_to_its_limit(alslib):
    """cumf_quadratic_sse_terms at the f of the gap and at its last f (256; one thread per column of a 256-thread workgroup)
    against the numpy fp64 formula of test_quadratic_sse_terms_kernel, same 2e-6 sum |q| bound, with a skipped system (reg < 0,
    NaN solution) and a reg == 0 system; f = 258 is refused."""
    _need_gpu()
    from cumf_als_amd import als

    rng = np.random.RandomState(0)
    dev = lambda a: torch.from_numpy(a).cuda()
    for f in (202, 206, 207, 256):
        batch = 37
        g = rng.standard_normal((batch, f, f + 5)).astype(np.float32)
        reg = (0.05 * rng.randint(1, 50, size=batch)).astype(np.float32)
        A = np.einsum("bik,bjk->bij", g, g).astype(np.float32) + reg[:, None, None] * np.eye(f, dtype=np.float32)
        b = rng.standard_normal((batch, f)).astype(np.float32)
        x = (0.1 * rng.standard_normal((batch, f))).astype(np.float32)
        reg[3] = -1.0
        x[3] = np.nan
        A[5] -= reg[5] * np.eye(f, dtype=np.float32)
        reg[5] = 0.0
        A64, b64, x64, r64 = (v.astype(np.float64) for v in (A, b, x, reg))
        q = 2.0 * (x64 * b64).sum(1) - np.einsum("bi,bij,bj->b", x64, A64, x64) + r64 * (x64 * x64).sum(1)
        want = q[reg >= 0].sum()
        got = float(als.quadratic_sse_terms(dev(A), dev(b), dev(x), dev(reg)).item())
        scale = np.abs(q[reg >= 0]).sum()
        print(f"quadratic terms f={f}: |got - want| / sum|q| = {abs(got - want) / scale:.3e}")
        assert abs(got - want) <= 2e-6 * scale, (f, got, want)
    f = 258
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="cumf_quadratic_sse_terms"):
        als.quadratic_sse_terms(torch.zeros((2, f, f), device="cuda"), torch.ones((2, f), device="cuda"),
                                torch.ones((2, f), device="cuda"), torch.ones(2, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert float(out.item()) == 0.0


def _sse64(ptr, idx, val, table, x):
    """sum over the ratings of the systems with ratings of (r - table[user] . x[item])^2 and of r^2, in fp64."""
    t64, x64 = table.astype(np.float64), x.astype(np.float64)
    sse = s2 = 0.0
    for v in range(len(ptr) - 1):
        sl = slice(int(ptr[v]), int(ptr[v + 1]))
        if sl.stop > sl.start:
            r = val[sl].astype(np.float64)
            sse += float(((r - t64[idx[sl]] @ x64[v]) ** 2).sum())
            s2 += float((r * r).sum())
    return sse, s2


@pytest.mark.parametrize("f", [200, 202, 206])
@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_materialise_solve_terms_chain(alslib, solver, f):
    """The Theta update of the `reduce` scheme without a process group, on one plan: cumf_get_hermitian_packed ->
    cumf_unpack_upper -> batched solver -> cumf_quadratic_sse_terms on the SAME unpacked batch (reg = lambda n_v, -1 for the
    item without ratings).  sum r^2 - terms must be the fp64 sum of squared errors of the returned factors over the ratings to
    2e-5 (the bound of test_distals_train_sse_out_of_the_theta_update for this identity), and the unpacked batch and the
    right-hand sides must keep their bits across the solve."""
    _need_gpu()
    from cumf_als_amd import als

    ptr, idx, val = _item_side()
    table = _factors(USERS, f, 1)
    lens = np.diff(ptr)
    reg = np.where(lens > 0, np.float32(LAM) * lens.astype(np.float32), np.float32(-1.0)).astype(np.float32)
    plan = als.Plan(ptr, f)
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # a copy: the shared set is read-only
    packed, rhs = als.get_hermitian_packed(plan, dev(idx), dev(val), dev(table), LAM)
    full = torch.empty((len(lens), f, f), device="cuda")
    als.unpack_upper(packed, full)
    torch.cuda.synchronize()
    a_bits, b_bits = _bits(full), _bits(rhs)
    if solver == "lu":
        x = als.lu_solve(full, rhs)
    else:
        x = als.cg_solve(full, torch.zeros_like(rhs), rhs, 6)
    terms = als.quadratic_sse_terms(full, rhs, x, dev(reg))
    torch.cuda.synchronize()
    a_kept, b_kept = _same_bits(full, a_bits), _same_bits(rhs, b_bits)
    sse, s2 = _sse64(ptr, idx, val, table, x.cpu().numpy())
    got = s2 - float(terms.item())
    print(f"chain {solver} f={f}: batch intact {a_kept}, rhs intact {b_kept}; sum r^2 = {s2:.1f}, SSE from the terms {got:.4f}, "
          f"fp64 over the ratings {sse:.4f}, rel {abs(got - sse) / sse:.2e}")
    assert sse >= 1e-2 * s2, (sse, s2)  # the identity is not cancellation noise
    assert a_kept, "the solver modified the unpacked batch"
    assert b_kept, "the solver modified the right-hand sides"
    assert abs(got - sse) <= 2e-5 * sse, (got, sse)


DIST_M, DIST_N, DIST_NNZ, DIST_LAM = 600, 40, 12000, 0.2


def _train_sse64(d, thetaT, XT):
    t64, x64 = thetaT.astype(np.float64), XT.astype(np.float64)
    r = d["csr_data"].astype(np.float64)
    return float(((r - (x64[d["coo_row"]] * t64[d["csr_indices"]]).sum(1)) ** 2).sum()), float((r * r).sum())


@pytest.mark.parametrize("f", [200, 204])
@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_reduce_scheme_train_sse_in_the_gap(alslib, solver, f):
    """DistALS `reduce` scheme, one rank, no process group, the collectives driven from Python (dist.py: unpack -> solve ->
    quad_terms on its `_my_tt`): update_theta(train_sse=True) at the last f of the register LU and inside the gap, against
    the RMSE kernel over the ratings to 2e-5.  600 x 40, 12 000 ratings: every item has ~190 .. 400 ratings, every user ~20, so
    the X side fits almost perfectly; lambda = 0.2 leaves SSE = 0.07 sum r^2 after one iteration on the CPU oracle
    (0.007 at lambda = 0.05), asserted below in fp64 on the returned factors."""
    _need_gpu()
    from cumf_als_amd import als, datagen
    from cumf_als_amd import dist as cdist

    r = datagen.synth_ratings(DIST_M, DIST_N, DIST_NNZ, 300, seed=7).to("cuda")
    theta0 = _factors(r.n, f, 0)
    cdist.set_native(False)
    try:
        eng = cdist.DistALS.from_local_slab(r.m, r.n, np.array([0, r.m], dtype=np.int64), r.csr_indptr, r.csr_indices,
                                            r.csr_data, f, DIST_LAM, cdist.HipOps(torch.device("cuda")), solver=solver,
                                            theta_batch=3)
    finally:
        cdist.set_native(None)
    assert eng._nr is None
    eng.init_factors(theta0)
    eng.update_x()
    got = eng.update_theta(train_sse=True)
    torch.cuda.synchronize()
    want = float(als.sse(r.csr_data, r.coo_row, r.csr_indices, eng.thetaT, eng.full_XT()).item())
    sse, s2 = _train_sse64(r.numpy(), eng.thetaT.cpu().numpy(), eng.full_XT().cpu().numpy())
    print(f"DistALS reduce {solver} f={f}: train SSE from the Theta update {got}, RMSE kernel {want:.4f}, fp64 {sse:.4f}, "
          f"sum r^2 {s2:.1f}")
    eng.close()
    assert sse >= 1e-2 * s2, (sse, s2)
    assert got is not None
    assert abs(got - want) <= 2e-5 * want, (got, want)


def _native_reduce_worker(port, solver, d, m, n, f, lam, theta0, q):
    """One rank over RCCL, CUMF_DIST_NATIVE=1: the Theta update is one call of cumf_dist_reduce_update_theta (als_dist.cpp)."""
    import os

    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["CUMF_DIST_NATIVE"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from cumf_als_amd import dist as cdist

        mat = cdist.HostMatrix(m, n, d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indptr"], d["csc_indices"],
                               d["csc_data"])
        eng = cdist.DistALS(mat, f, lam, cdist.HipOps("cuda:0"), solver=solver, cg_iters=6, scheme="reduce", theta_batch=3)
        assert eng._ncomm is not None and eng._ncomm.name == "rccl" and eng._nr is not None
        eng.init_factors(theta0)
        eng.update_x()
        sse = eng.update_theta(train_sse=True)
        torch.cuda.synchronize()
        q.put((sse, eng.thetaT.cpu().numpy().copy(), eng.full_XT().cpu().numpy().copy()))
    except BaseException as e:  # the parent reports it instead of waiting for a result that never comes
        q.put(repr(e))
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_native_reduce_train_sse_in_the_gap(alslib, solver):
    """The same through cumf_dist_reduce_update_theta (unpack -> cumf_lu_solve_batched / cumf_cg_solve_batched ->
    cumf_quadratic_sse_terms on its `my_tt`) at f = 204, one rank over RCCL in a fresh process: the train SSE it returns
    against the fp64 SSE of the factors it returns, to 2e-5."""
    _need_gpu()
    import torch.multiprocessing as mp

    from cumf_als_amd import datagen
    from tests.test_dist_cpu import _free_port

    f = 204
    d = datagen.synth_ratings(DIST_M, DIST_N, DIST_NNZ, 300, seed=7).numpy()
    theta0 = _factors(DIST_N, f, 0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_native_reduce_worker, args=(_free_port(), solver, d, DIST_M, DIST_N, f, DIST_LAM, theta0, q))
    import queue

    p.start()
    out = None
    while out is None:  # ends with the child, whichever way it goes
        try:
            out = q.get(timeout=1.0)
        except queue.Empty:
            assert p.is_alive() or not q.empty(), f"the worker died without a result (exit code {p.exitcode})"
    p.join(timeout=120)
    assert not isinstance(out, str), out
    assert p.exitcode == 0
    got, th, x = out
    sse, s2 = _train_sse64(d, th, x)
    print(f"native reduce {solver} f={f}: train SSE from the Theta update {got}, fp64 {sse:.4f}, sum r^2 {s2:.1f}")
    assert sse >= 1e-2 * s2, (sse, s2)
    assert got is not None
    assert abs(got - sse) <= 2e-5 * sse, (got, sse)
