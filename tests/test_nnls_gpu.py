"""Non-negative least squares and non-negative ALS on the MI355X (include/cumf_nnls_capi.h) against the fp64 reference of
tests/nnls_ref.py.

Tolerances.  For a returned x of the system (A, b): s = max|b| + max|A| max|x|, g = A x - b in fp64 from the fp32 inputs,
  KKT       min x >= 0 exactly, g_i >= -tau everywhere, |g_i| <= tau where x_i > 0, tau = 4 f 2^-24 s;
  distance  |x - x*|_inf <= 2 |x_lu32 - x*|_inf + 1e-5 |x*|_inf, x_lu32 the fp32 oracle LU of the reference's final
            masked system (the bound of the implicit LU tests).
"""
import numpy as np
import pytest
import torch

from tests import implicit_ref
from tests import nnls_ref as ref

pytestmark = pytest.mark.gpu

FS = [1, 8, 10, 16, 32, 50, 64, 100, 128]
LENS = [0, 1, 7, 31, 32, 33, 64, 65, 500, 20000]
N_COLS = 24000


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stats():
    return torch.zeros(2, dtype=torch.int64, device="cuda")


def _solve(A, b, x0, max_iters=0):
    from cumf_als_amd import als

    Ag, bg, xg, st = _dev(A), _dev(b), _dev(x0), _stats()
    als.nnls_solve(Ag, bg, xg, max_iters, st)
    torch.cuda.synchronize()
    return xg.cpu().numpy(), st.cpu().numpy(), Ag, bg


def _assert_kkt(A, b, x, what):
    A64, b64, x64 = A.astype(np.float64), b.astype(np.float64), x.astype(np.float64)
    f = b.shape[-1]
    assert (x >= 0).all(), (what, x.min())
    g = np.einsum("bij,bj->bi", A64, x64) - b64
    s = np.abs(b64).max(1) + np.abs(A64).max((1, 2)) * np.abs(x64).max(1)
    tau = (4 * f * 2.0 ** -24 * s)[:, None]
    assert (g >= -tau).all(), (what, (g / tau).min())
    assert (np.abs(np.where(x > 0, g, 0)) <= tau).all(), (what, np.abs(np.where(x > 0, g, 0) / tau).max())


def _assert_distance(oracle, A, b, x, what):
    """Per system against the reference, with the fp32 oracle LU of the reference's final masked system as yardstick."""
    f = b.shape[-1]
    xs, Fs = ref.nnls_batch(A, b)
    Am = np.empty_like(A)
    bm = np.empty_like(b)
    for k in range(len(b)):
        Am[k], bm[k] = ref.masked_system(A[k], b[k], Fs[k])
    x_lu = oracle.lu(Am.astype(np.float32), bm.astype(np.float32), f)
    e_h = np.abs(x - xs).max(1)
    e_o = np.abs(x_lu - xs).max(1)
    bound = 2 * e_o + 1e-5 * np.abs(xs).max(1)
    assert (e_h <= bound).all(), (what, e_h.max(), e_o.max(), int(np.argmax(e_h - bound)))
    return xs, Fs


@pytest.mark.parametrize("f", FS)
def test_nnls_solve_batched(oracle, alslib, f):
    rng = np.random.RandomState(f)
    batch = 64
    A = ref.random_spd(rng, batch, f)
    b = rng.standard_normal((batch, f)).astype(np.float32)  # about half of each unconstrained solution negative
    A0, b0 = A.copy(), b.copy()
    x, st, Ag, bg = _solve(A, b, np.zeros_like(b))  # cold start
    _assert_kkt(A, b, x, f"cold f={f}")
    xs, Fs = _assert_distance(oracle, A, b, x, f"cold f={f}")
    assert st[0] == 0, st
    assert torch.equal(Ag.cpu(), torch.from_numpy(A0)) and torch.equal(bg.cpu(), torch.from_numpy(b0))  # not modified
    x2, st2, _, _ = _solve(A, b, np.zeros_like(b))
    assert np.array_equal(x.view(np.int32), x2.view(np.int32)) and np.array_equal(st, st2)  # bit-identical runs
    # warm start from x*: one factorisation per system with a non-empty support
    xw, stw, _, _ = _solve(A, b, xs.astype(np.float32))
    _assert_kkt(A, b, xw, f"warm f={f}")
    _assert_distance(oracle, A, b, xw, f"warm f={f}")
    assert stw[0] == 0 and stw[1] == int(Fs.any(1).sum()), (stw, int(Fs.any(1).sum()))
    print(f"nnls f={f}: cold {st[1] / batch:.2f} factorisations per system, warm {stw[1] / batch:.2f}")


@pytest.mark.parametrize("f", FS)
def test_nnls_positive_and_nonpositive_cases(oracle, alslib, f):
    from cumf_als_amd import als

    rng = np.random.RandomState(50 + f)
    batch = 32
    A = ref.random_spd(rng, batch, f)
    x0 = rng.uniform(0.5, 2.0, (batch, f))
    b = np.einsum("bij,bj->bi", A.astype(np.float64), x0).astype(np.float32)  # all-positive unconstrained solutions
    x, st, Ag, bg = _solve(A, b, np.zeros_like(b))
    assert st[0] == 0
    x_lu = als.lu_solve(Ag, bg).cpu().numpy()
    xs = np.linalg.solve(A.astype(np.float64), b.astype(np.float64)[..., None])[..., 0]
    x32 = oracle.lu(A, b, f)
    bound = 2 * np.abs(x32 - xs).max(1) + 1e-5 * np.abs(xs).max(1)
    assert (np.abs(x - x_lu).max(1) <= bound).all(), (f, np.abs(x - x_lu).max())
    assert (np.abs(x - xs).max(1) <= bound).all(), (f, np.abs(x - xs).max())
    bn = -np.abs(rng.standard_normal((batch, f))).astype(np.float32)  # b <= 0: exactly 0, from any start
    for start in (np.zeros_like(bn), rng.uniform(0, 1, (batch, f)).astype(np.float32)):
        x, st, _, _ = _solve(A, bn, start)
        assert st[0] == 0 and not x.any(), (f, st, np.abs(x).max())


def test_nnls_large_batch(alslib):
    """More systems than 65 535, f = 8: the grid-stride loop covers them all."""
    rng = np.random.RandomState(3)
    batch, f = 70001, 8
    A = ref.random_spd(rng, batch, f)
    b = rng.standard_normal((batch, f)).astype(np.float32)
    x, st, _, _ = _solve(A, b, np.zeros_like(b))
    assert st[0] == 0
    _assert_kkt(A, b, x, "large batch")
    for k in list(range(0, batch, 9973)) + [batch - 1]:  # spot checks against the reference
        xs, _ = ref.nnls(A[k], b[k])
        assert np.abs(x[k] - xs).max() <= 1e-4 * max(1.0, np.abs(xs).max()), k


def test_nnls_not_spd_rows_end_and_are_counted(alslib):
    rng = np.random.RandomState(4)
    f, batch = 32, 8
    A = ref.random_spd(rng, batch, f)
    b = rng.standard_normal((batch, f)).astype(np.float32)
    A[2] = 0  # zero matrix, mixed b: the positive entries enter the passive set, whose solve is not finite
    A[5, 3, 3] = np.nan
    x, st, _, _ = _solve(A, b, np.zeros_like(b))
    assert st[0] == 2, st
    ok = [k for k in range(batch) if k not in (2, 5)]
    _assert_kkt(A[ok], b[ok], x[ok], "SPD rows next to bad ones")
    # a cap of one step: rows that need more are counted, none faults
    x1, st1, _, _ = _solve(A[ok], b[ok], np.zeros_like(b[ok]), max_iters=1)
    assert st1[0] == len(ok) and (x1 >= 0).all(), st1


# ---------------------------------------------------------------------------------------------------------------------
# half-iteration routes
# ---------------------------------------------------------------------------------------------------------------------

def _mixed(seed=7):
    """One plan of every interesting row length, the 20 000-entry row chunked by the plan."""
    rng = np.random.RandomState(seed)
    lens = LENS + [0, 1, 7, 33, 65] + list(rng.randint(1, 120, 5))
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(N_COLS, ln, replace=False)) for ln in lens]).astype(np.int32)
    val = rng.choice(np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32), int(rowptr[-1]))
    return lens, rowptr, colidx, val


def _table(f, seed):
    # mixed-sign factors: the unconstrained solutions have negative entries
    return (0.3 * np.random.RandomState(seed).standard_normal((N_COLS, f))).astype(np.float32)


def _explicit_systems(rowptr, colidx, val, Y, lam):
    Y = Y.astype(np.float64)
    f = Y.shape[1]
    rows = len(rowptr) - 1
    A = np.zeros((rows, f, f))
    b = np.zeros((rows, f))
    for u in range(rows):
        s, e = rowptr[u], rowptr[u + 1]
        yu = Y[colidx[s:e]]
        A[u] = yu.T @ yu + lam * (e - s) * np.eye(f)
        b[u] = val[s:e].astype(np.float64) @ yu
    return A, b


def _check_route(oracle, lens, A64, b64, x, what):
    empty = np.asarray(lens) == 0
    assert (x >= 0).all(), (what, x.min())
    assert not x[empty].any(), what
    ne = ~empty
    _assert_distance(oracle, A64[ne], b64[ne], x[ne], what)


@pytest.mark.parametrize("gram_mode", ["exact", "auto"], indirect=True)
@pytest.mark.parametrize("f", [8, 32, 64, 100, 128])
def test_update_nonneg_explicit(oracle, alslib, gram_mode, f):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _mixed()
    Y = _table(f, 3)
    lam = 0.05
    A64, b64 = _explicit_systems(rowptr, colidx, val, Y, lam)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)  # warm start, mixed signs
    for rp in ([rowptr, rowptr.astype(np.int64)] if f == 64 else [rowptr]):
        plan = als.Plan(rp, f)
        assert plan.n_multi_rows >= 1
        x, st = _dev(x0), _stats()
        als.update_nonneg(plan, _dev(colidx), _dev(val), _dev(Y), x, lam, stats=st)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        _check_route(oracle, lens, A64, b64, xh, f"explicit f={f} {gram_mode} {rp.dtype}")
        assert st[0].item() == 0, st
        plan.close()


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("f", [8, 32, 64, 100, 128])
def test_update_nonneg_implicit(oracle, alslib, f, reg):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _mixed(11)
    val = (val - 2.0).astype(np.float32)  # negatives and stored zeros
    Y = _table(f, 5)
    lam, alpha = 0.05, 40.0 if reg == "weighted" else 1.0
    A64, b64 = implicit_ref.systems(rowptr, colidx, val, Y, lam, alpha, reg)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
    plan = als.Plan(rowptr, f)
    Yg = _dev(Y)
    x, st = _dev(x0), _stats()
    als.update_implicit_nonneg(plan, _dev(colidx), _dev(val), Yg, als.implicit_gram(Yg), x, lam, alpha, reg, stats=st)
    torch.cuda.synchronize()
    _check_route(oracle, lens, A64, b64, x.cpu().numpy(), f"implicit f={f} {reg}")
    assert st[0].item() == 0, st


# ---------------------------------------------------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine_data():
    from cumf_als_amd import datagen

    return datagen.synth_ratings(3000, 800, 120_000, 2000, seed=5).to("cuda")


def _explicit_objective(d, X, T, lam):
    X, T = X.astype(np.float64), T.astype(np.float64)
    rowptr, col, r = d["csr_indptr"].astype(np.int64), d["csr_indices"], d["csr_data"].astype(np.float64)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    pred = np.einsum("ij,ij->i", X[row], T[col])
    nu, nv = np.diff(rowptr), np.bincount(col, minlength=T.shape[0])
    return float(((r - pred) ** 2).sum() + lam * (nu * (X ** 2).sum(1)).sum() + lam * (nv * (T ** 2).sum(1)).sum())


def _check_engine(e, objective, what):
    prev = None
    values = []
    for _ in range(5):
        for half in (e.update_x, e.update_theta):
            half()
            torch.cuda.synchronize()
            assert (e.XT >= 0).all() and (e.thetaT >= 0).all(), what
            cur = objective()
            values.append(cur)
            if prev is not None:
                assert cur <= prev + 1e-6 * abs(prev), (what, values)
            prev = cur
    assert e.nnls_stats[0].item() == 0, (what, e.nnls_stats)
    ids, _ = e.recommend(10)
    ids = ids.cpu().numpy()
    assert ((ids >= 0) & (ids < e.n)).all(), what
    print(f"{what}: objective {values[0]:.6g} -> {values[-1]:.6g}, stats {e.nnls_stats.tolist()}, "
          f"zero share X {float((e.XT == 0).float().mean()):.3f}")


def test_engine_explicit_nonneg(engine_data):
    from cumf_als_amd import als

    d = engine_data.numpy()
    e = als.ALSEngine(engine_data, 32, 0.05, nonnegative=True)
    e.init_factors(seed=1)
    _check_engine(e, lambda: _explicit_objective(d, e.XT.cpu().numpy(), e.thetaT.cpu().numpy(), 0.05), "explicit")
    e.close()


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_engine_implicit_nonneg(engine_data, reg):
    from cumf_als_amd import als

    e = als.ImplicitALSEngine(engine_data, 32, 0.05, 40.0, reg=reg, nonnegative=True)
    e.init_factors(seed=1)
    _check_engine(e, e.loss, f"implicit {reg}")
    e.close()


def test_engines_nonnegative_false_is_the_default(engine_data):
    from cumf_als_amd import als

    for make in (lambda **kw: als.ALSEngine(engine_data, 32, 0.05, solver="lu", **kw),
                 lambda **kw: als.ImplicitALSEngine(engine_data, 32, 0.05, 40.0, solver="cg", **kw)):
        a, b = make(), make(nonnegative=False)
        for e in (a, b):
            e.init_factors(seed=2)
            e.iterate(2)
        torch.cuda.synchronize()
        assert torch.equal(a.XT, b.XT) and torch.equal(a.thetaT, b.thetaT)
        assert not hasattr(b, "nnls_stats") or not b.nnls_stats.any()
        a.close()
        b.close()
