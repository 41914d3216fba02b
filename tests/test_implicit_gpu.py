"""Implicit-feedback ALS on the MI355X (include/cumf_implicit_capi.h) against the numpy reference of tests/implicit_ref.py,
solved by the oracle's own CG / LU in fp32 and fp64."""
import numpy as np
import pytest
import torch

from tests import implicit_ref as ref

pytestmark = pytest.mark.gpu

LENS = [0, 1, 7, 31, 32, 33, 64, 65, 500, 20000]
N_COLS = 24000


def _mixed(seed=7):
    """One plan of every interesting row length (twice, plus a few random ones); ratings with negatives and stored zeros."""
    rng = np.random.RandomState(seed)
    lens = LENS + [0, 1, 7, 31, 32, 33, 64, 65, 500] + list(rng.randint(1, 120, 13))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(N_COLS, ln, replace=False)) for ln in lens]).astype(np.int32)
    val = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0], np.float32), int(rowptr[-1]))
    return lens, rowptr, colidx, val


def _table(rows, f, seed):
    return (0.3 * np.random.RandomState(seed).standard_normal((rows, f))).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("f", [8, 10, 32, 50, 64, 100, 128])
def test_implicit_gram(alslib, f):
    from cumf_als_amd import als

    for rows in (1, 1000, 3001):  # below, and not a multiple of, the 1024-row slab and the 32-row stage
        Y = _table(rows, f, rows + f)
        G = als.implicit_gram(_dev(Y))
        G2 = als.implicit_gram(_dev(Y))
        torch.cuda.synchronize()
        g, g2 = G.cpu().numpy(), G2.cpu().numpy()
        Y64 = Y.astype(np.float64)
        err = np.abs(g - Y64.T @ Y64)
        assert (err <= 1e-5 * (np.abs(Y64).T @ np.abs(Y64))).all(), (f, rows, err.max())
        assert np.array_equal(g, g2) and np.array_equal(g, g.T), (f, rows)


@pytest.mark.parametrize("f", [10, 50, 100, 128])
def test_get_hermitian_implicit(alslib, f):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _mixed()
    Y = _table(N_COLS, f, 3)
    plan = als.Plan(rowptr, f)
    assert plan.n_multi_rows >= 1  # the 20 000-entry row is cut into chunks
    cg, vg, Yg = _dev(colidx), _dev(val), _dev(Y)
    G = als.implicit_gram(Yg)
    for alpha in (1.0, 40.0):
        for reg in ("weighted", "plain"):
            tt, rhs = als.get_hermitian_implicit(plan, cg, vg, Yg, G, 0.05, alpha, reg)
            tt2, rhs2 = als.get_hermitian_implicit(plan, cg, vg, Yg, G, 0.05, alpha, reg)
            torch.cuda.synchronize()
            A64, b64 = ref.systems(rowptr, colidx, val, Y, 0.05, alpha, reg)
            Aabs, babs = ref.systems(rowptr, colidx, val, Y, 0.05, alpha, reg, absolute=True)
            t, r = tt.cpu().numpy(), rhs.cpu().numpy()
            assert (np.abs(t - A64) <= 1e-5 * Aabs).all(), (f, alpha, reg, np.abs(t - A64).max())
            cabs = ref.rhs_scale(rowptr, colidx, val, Y, alpha)  # |b| formula: sum (1 + w) |y| over the positive entries
            assert (np.abs(r - b64) <= 1e-5 * cabs + 1e-30).all(), (f, alpha, reg, np.abs(r - b64).max())
            assert torch.equal(tt, tt2) and torch.equal(rhs, rhs2)


def _route_case(f, alpha, reg, seed=7):
    lens, rowptr, colidx, val = _mixed(seed)
    Y = _table(N_COLS, f, 3)
    A64, b64 = ref.systems(rowptr, colidx, val, Y, 0.05, alpha, reg)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
    return lens, rowptr, colidx, val, Y, A64, b64, x0


def _update(rowptr, colidx, val, Y, x0, f, alpha, reg, solver, iters):
    from cumf_als_amd import als

    plan = als.Plan(rowptr, f)
    Yg = _dev(Y)
    x = _dev(x0.copy())
    als.update_implicit(plan, _dev(colidx), _dev(val), Yg, als.implicit_gram(Yg), x, 0.05, alpha, reg, solver, iters)
    torch.cuda.synchronize()
    return x.cpu().numpy(), als.last_kernel_name()


@pytest.mark.parametrize("f", [8, 64, 100, 128])
def test_update_implicit_lu(oracle, alslib, f):
    lens = None
    for alpha, reg in ((1.0, "weighted"), (40.0, "plain")):
        lens, rowptr, colidx, val, Y, A64, b64, x0 = _route_case(f, alpha, reg)
        x, _ = _update(rowptr, colidx, val, Y, x0, f, alpha, reg, "lu", 0)
        x64 = np.linalg.solve(A64, b64[..., None])[..., 0]
        x32 = oracle.lu(A64.astype(np.float32), b64.astype(np.float32), f)
        empty = np.asarray(lens) == 0
        assert (x[empty] == 0).all()
        e_h = np.abs(x - x64).max(1)[~empty]
        e_o = np.abs(x32 - x64).max(1)[~empty]
        scale = np.abs(x64).max()
        assert (e_h <= 2 * e_o + 1e-5 * scale).all(), (f, alpha, reg, e_h.max(), e_o.max())


@pytest.mark.parametrize("f", [10, 64, 100, 128])
@pytest.mark.parametrize("iters", [1, 3, 8])
def test_update_implicit_cg(oracle, alslib, f, iters):
    stats = lambda v: (float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max()))
    for alpha, reg in ((40.0, "weighted"), (1.0, "plain")):
        lens, rowptr, colidx, val, Y, A64, b64, x0 = _route_case(f, alpha, reg)
        x, name = _update(rowptr, colidx, val, Y, x0, f, alpha, reg, "cg", iters)
        assert "implicit_short_cg_kernel" in name, name  # rows of at most 32 entries took the Gram-free kernel
        x64 = oracle.cg(A64, x0.astype(np.float64), b64, f, iters)
        x32 = oracle.cg(A64.astype(np.float32), x0, b64.astype(np.float32), f, iters)
        empty = np.asarray(lens) == 0
        assert (x[empty] == 0).all()
        e_h = np.abs(x - x64).max(1)[~empty]
        e_o = np.abs(x32 - x64).max(1)[~empty]
        scale = np.abs(x64).max()
        print(f"implicit CG f={f} iters={iters} alpha={alpha}: hip {stats(e_h)} oracle32 {stats(e_o)}")
        for sh, so in zip(stats(e_h), stats(e_o)):
            assert sh <= 1.05 * so + 1e-5 * scale, (f, iters, alpha, stats(e_h), stats(e_o))
    # the LU route never runs the Gram-free kernel
    _, name = _update(rowptr, colidx, val, Y, x0, f, 40.0, "weighted", "lu", 0)
    assert "implicit_short_cg_kernel" not in name, name


@pytest.fixture(scope="module")
def engine_data():
    from cumf_als_amd import datagen

    r = datagen.synth_ratings(20000, 5000, 2_000_000, 1000, seed=5)
    # interaction strengths with negatives and stored zeros: 1..5 -> -1..3
    r.csr_data.sub_(2.0)
    r.csc_data.sub_(2.0)
    return r.to("cuda")


def _engine(r, solver, theta_batch=1, reg="weighted"):
    from cumf_als_amd import als

    e = als.ImplicitALSEngine(r, 64, 0.05, 40.0, solver=solver, cg_iters=3, reg=reg, theta_batch=theta_batch)
    e.init_factors(seed=1)
    return e


def test_engine_loss_matches_numpy(engine_data):
    r = engine_data
    d = r.to("cpu")
    for reg in ("weighted", "plain"):
        e = _engine(r, "lu", reg=reg)
        e.update_x()
        got = e.loss()
        want = ref.sparse_loss(d.csr_indptr.numpy(), d.csr_indices.numpy(), d.csr_data.numpy(), e.XT.cpu().numpy(),
                               e.thetaT.cpu().numpy(), 0.05, 40.0, reg)
        e.close()
        assert abs(got - want) <= 1e-6 * abs(want), (reg, got, want)


@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_engine_loss_is_non_increasing(engine_data, solver):
    e = _engine(engine_data, solver)
    e.update_x()
    prev = e.loss()
    losses = [prev]
    for _ in range(5):
        for half in (e.update_theta, e.update_x):
            half()
            cur = e.loss()
            losses.append(cur)
            assert cur <= prev + 1e-6 * abs(prev), (solver, losses)
            prev = cur
    e.close()
    print(f"implicit {solver} losses: {losses}")


def test_engine_theta_batches_are_bit_identical(engine_data):
    e1, e3 = _engine(engine_data, "cg", 1), _engine(engine_data, "cg", 3)
    e1.iterate(2)
    e3.iterate(2)
    torch.cuda.synchronize()
    assert torch.equal(e1.thetaT, e3.thetaT) and torch.equal(e1.XT, e3.XT)
    e1.close()
    e3.close()
