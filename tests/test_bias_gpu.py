"""Biased explicit ALS on the MI355X (include/cumf_bias_capi.h) against numpy fp32 bit for bit where the header fixes the
arithmetic, against the plain fused update bit for bit where it promises the same kernels, and against the fp64 reference of
tests/bias_ref.py elsewhere.  The data is the planted set of bias_ref (300 x 200, 7 184 ratings, row 5 and column 9 empty)
or smaller."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bias_ref as ref

pytestmark = pytest.mark.gpu

LAM = 0.05


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ratings(data):
    """datagen.Ratings on the device from (R, train, test) of bias_ref."""
    from cumf_als_amd import datagen

    R, train, test = data
    tr, tc = np.nonzero(train)
    er, ec = np.nonzero(test)
    return datagen.from_coo(R.shape[0], R.shape[1], tr, tc, R[train].astype(np.float32), er, ec,
                            R[test].astype(np.float32)).to("cuda")


@pytest.fixture(scope="module")
def planted():
    data = ref.planted_bias_ratings()
    return data, _ratings(data)


@pytest.fixture(scope="module")
def reference():
    """bias_ref.run(10) at f = 8, lambda = lambda_bias = 0.05: computed once, shared, never modified."""
    return ref.run(10, 8, LAM)


def _start(m, n, f, seed=3):
    """Nonzero factors and biases for both sides (fp32)."""
    rng = np.random.RandomState(seed)
    return ((0.2 * rng.random_sample((n, f))).astype(np.float32), (0.1 * rng.standard_normal((m, f))).astype(np.float32),
            (0.3 * rng.standard_normal(m)).astype(np.float32), (0.3 * rng.standard_normal(n)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the residual kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1025, 7184])
def test_residual_kernel_bits(alslib, count, offset):
    """(val - mu) - bias[idx] in fp32, two roundings: every length around the 16-byte body, every misalignment of the
    first entry, one NaN bias (which gives NaN exactly where it is gathered); the entries around the call's range stay
    untouched."""
    from cumf_als_amd import als

    rng = np.random.RandomState(count + offset)
    nb = 200
    val = (3.5 + rng.standard_normal(count + offset + 8)).astype(np.float32)
    idx = rng.randint(0, nb, count + offset + 8).astype(np.int32)
    bias = (0.5 * rng.standard_normal(nb)).astype(np.float32)
    bias[17] = np.nan
    idx[offset] = 17
    mu = 3.4567
    vg, ig, bg = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(bias).cuda()
    out = torch.full((count + offset + 8,), -7.0, dtype=torch.float32, device="cuda")
    als.residual_biased(vg[offset:offset + count], ig[offset:offset + count], bg, mu, out[offset:offset + count])
    torch.cuda.synchronize()
    want = np.full(count + offset + 8, -7.0, np.float32)
    want[offset:offset + count] = (val[offset:offset + count] - np.float32(mu)) - bias[idx[offset:offset + count]]
    got = out.cpu().numpy()
    # a NaN stays a NaN in the same place (IEEE 754 leaves the sign and payload of a propagated NaN to the implementation:
    # numpy on the host and v_sub_f32 on the device need not agree on them); every other entry is compared bit for bit
    nan = np.isnan(want)
    assert nan[offset] and nan.sum() == (idx[offset:offset + count] == 17).sum()
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero((_bits(got) != _bits(want)) & ~nan)
    assert bad.size == 0, (bad[:8], [hex(v) for v in _bits(got)[bad[:8]]], [hex(v) for v in _bits(want)[bad[:8]]])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the half-iteration against a hand-built plain call, on every kernel route
# ---------------------------------------------------------------------------------------------------------------------
def _hand_half(plans, colidx, val, gather_f, gather_b, own_f, own_b, own, other, s, mu, lam, solver):
    """[gather_f | s | 0] (columns own | other), [own_f | own_b / s | 0] and r' in numpy fp32, then als.update_fused on each
    plan: the updated table as numpy."""
    from cumf_als_amd import als

    F = gather_f.shape[1] + 2
    gather = np.zeros((gather_f.shape[0], F), np.float32)
    gather[:, :F - 2], gather[:, own], gather[:, other] = gather_f, s, 0.0
    update = np.zeros((own_f.shape[0], F), np.float32)
    update[:, :F - 2], update[:, own], update[:, other] = own_f, own_b / s, 0.0
    rp = (val.cpu().numpy() - np.float32(mu)) - gather_b[colidx.cpu().numpy()]
    assert rp.dtype == np.float32 and update.dtype == np.float32
    g, u, rpg = torch.from_numpy(gather).cuda(), torch.from_numpy(update).cuda(), torch.from_numpy(rp).cuda()
    for p in plans:
        als.update_fused(p, colidx, rpg, g, u, lam, solver, 6)
    torch.cuda.synchronize()
    return u.cpu().numpy()


# The decoupled unknown of the plain call is 0 in exact arithmetic.  At F = 16 and 64 the wave kernels return a term of
# denormal size instead (5e-42 at most, measured; the doubled h plane of their diagonal Gram tiles makes 2^-126 of a zero of
# the gather table); the biased call overwrites that column either way.
TINY = 1e-36
ROUTES = [(8, 0), (14, 0), (62, 0), (98, 0), (110, 0), (204, 0), (14, 32), (98, 32)]  # (f, chunk): F = 10 .. 206


@pytest.mark.parametrize("solver", ["lu", "cg"])
@pytest.mark.parametrize("f,chunk", ROUTES)
def test_half_iteration_equals_the_plain_call_at_F(alslib, planted, f, chunk, solver):
    from cumf_als_amd import als

    _, r = planted
    F, m, n = f + 2, r.m, r.n
    th0, x0, b0, c0 = _start(m, n, f)
    plain = als.ALSEngine(r, F, LAM, solver, 6, x_batch=2, theta_batch=3, chunk=chunk)  # plans cut by the engine's rule, at F
    for lam_b in (LAM, LAM / 4, 0.02):
        s = np.float32(np.sqrt(np.float64(np.float32(LAM)) / np.float64(np.float32(lam_b))))
        if lam_b == LAM / 4:
            assert s == 2.0
        eng = als.BiasedALSEngine(r, f, LAM, lam_b, solver=solver, cg_iters=6, x_batch=2, theta_batch=3, chunk=chunk)
        mu = eng.mu
        runs = []
        for _ in range(2):
            eng.init_factors(th0, x0, b0, c0)
            assert _same(eng.XT[:, f].cpu(), b0) and _same(eng.thetaT[:, f + 1].cpu(), c0)
            eng.update_x()
            torch.cuda.synchronize()
            XT, TT = eng.XT.cpu().numpy(), eng.thetaT.cpu().numpy()
            ub, ib = eng.user_bias.cpu().numpy(), eng.item_bias.cpu().numpy()
            if not runs:
                z = _hand_half(plain.x_plans, r.csr_indices, r.csr_data, th0, c0, x0, b0, f, f + 1, s, mu, LAM, solver)
                live = np.ones(m, bool)
                live[5] = False
                assert np.isfinite(z[live]).all() and np.abs(z[live, f + 1]).max() <= TINY
                assert _same(XT[live, :f], z[live, :f]), (f, solver, lam_b, "x factors")
                assert _same(ub[live], z[live, f] * s), (f, solver, lam_b, "user bias")
                assert (XT[5, :f] == 0).all() and ub[5] == 0
                assert _same(XT[:, f], ub) and (XT[:, f + 1] == 1).all()
                assert (TT[:, f] == 1).all() and _same(TT[:, f + 1], ib) and _same(ib, c0) and _same(TT[:, :f], th0)
            x1, b1 = XT[:, :f].copy(), ub.copy()
            eng.update_theta()
            torch.cuda.synchronize()
            XT2, TT2 = eng.XT.cpu().numpy(), eng.thetaT.cpu().numpy()
            ub2, ib2 = eng.user_bias.cpu().numpy(), eng.item_bias.cpu().numpy()
            if not runs:
                z = _hand_half(plain.t_plans, r.csc_indices, r.csc_data, x1, b1, th0, c0, f + 1, f, s, mu, LAM, solver)
                live = np.ones(n, bool)
                live[9] = False
                assert np.isfinite(z[live]).all() and np.abs(z[live, f]).max() <= TINY
                assert _same(TT2[live, :f], z[live, :f]), (f, solver, lam_b, "theta factors")
                assert _same(ib2[live], z[live, f + 1] * s), (f, solver, lam_b, "item bias")
                assert (TT2[9, :f] == 0).all() and ib2[9] == 0
                assert (TT2[:, f] == 1).all() and _same(TT2[:, f + 1], ib2)
                assert _same(XT2[:, f], ub2) and (XT2[:, f + 1] == 1).all() and _same(ub2, b1) and _same(XT2[:, :f], x1)
            runs.append((XT2, TT2, ub2, ib2))
        assert all(_same(a, b) for a, b in zip(*runs)), (f, solver, lam_b, "two runs differ")
        eng.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. against fp64 on a well-posed set
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_set():
    """m = 200, n = 150, density 0.5, every rating in the training set, no empty row or column: about 75 ratings per row and
    100 per column (at f = 62 a few rows have fewer ratings than F = 64; lambda n_u keeps their systems well-posed)."""
    data = ref.planted_bias_ratings(200, 150, 0.5, seed=11, empty=False, test_share=0.0)
    return data, _ratings(data)


@pytest.mark.parametrize("f", [8, 62])
def test_half_iterations_against_fp64(alslib, dense_set, f):
    """One X half and one Theta half from the same inputs, LU: max |[x | b] - direct_half| <= 1e-4 max |reference|, the
    project's fused-LU tolerance (test_fused_half_iteration)."""
    from cumf_als_amd import als

    (R, train, _), r = dense_set
    m, n = R.shape
    th0, x0, b0, c0 = _start(m, n, f, seed=5)
    R32 = R.astype(np.float32).astype(np.float64)  # the ratings the engine sees
    lam_b = LAM / 4
    eng = als.BiasedALSEngine(r, f, LAM, lam_b, solver="lu")
    lam32, lamb32 = float(np.float32(LAM)), float(np.float32(lam_b))
    for side in ("x", "theta"):
        eng.init_factors(th0, x0, b0, c0)
        if side == "x":
            eng.update_x()
            got = np.hstack([eng.XT[:, :f].cpu().numpy(), eng.user_bias.cpu().numpy()[:, None]])
            X, b = ref.direct_half(R32, train, eng.mu, th0.astype(np.float64), c0.astype(np.float64), lam32, lamb32)
        else:
            eng.update_theta()
            got = np.hstack([eng.thetaT[:, :f].cpu().numpy(), eng.item_bias.cpu().numpy()[:, None]])
            X, b = ref.direct_half(R32.T, train.T, eng.mu, x0.astype(np.float64), b0.astype(np.float64), lam32, lamb32)
        want = np.hstack([X, b[:, None]])
        err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        print(f"f = {f}, {side} side: max error {err:.3g}, max |reference| {scale:.3g}, ratio {err / scale:.3g}")
        assert err <= 1e-4 * scale, (f, side, err, scale)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end, 5. mu
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(alslib, planted):
    """BiasedALSEngine(f = 8, LU, lambda = lambda_bias = 0.05) after 10 iterations from the reference's theta0, the last Theta
    half with the fused train SSE: (engine, sse of that half or None)."""
    from cumf_als_amd import als

    (R, _, _), r = planted
    eng = als.BiasedALSEngine(r, 8, LAM, solver="lu")
    eng.init_factors(ref.theta0(r.n, 8).astype(np.float32))
    eng.iterate(9)
    eng.update_x()
    sse = eng.update_theta_with_train_sse()
    torch.cuda.synchronize()
    yield eng, sse
    eng.close()


def test_end_to_end_rmse(alslib, planted, trained, reference):
    """Train and test RMSE within 1e-4 of the fp64 reference (the project's RMSE parity); the fused train SSE agrees with
    rmse()'s to 2e-5 relative (test_fused_train_sse_matches_the_rmse_kernel); and the biased model at f = 8 reaches at most
    0.9 x the test RMSE of the plain engine at the same table width f = 10 (fp64: 0.2055 / 0.2615 = 0.79)."""
    from cumf_als_amd import als

    _, r = planted
    eng, sse = trained
    train, test = eng.rmse()
    print(f"biased f = 8: train {train:.6f} test {test:.6f}; fp64 {reference['train_rmse']:.6f} {reference['test_rmse']:.6f}")
    assert abs(train - reference["train_rmse"]) <= 1e-4 and abs(test - reference["test_rmse"]) <= 1e-4
    if sse is not None:
        want = float(eng.train_sse().item())
        print(f"fused train SSE {float(sse.item()):.9g}, cumf_bias_sse {want:.9g}")
        assert abs(float(sse.item()) - want) <= 2e-5 * want
    plain = als.ALSEngine(r, 10, LAM, solver="lu")
    plain.init_factors(ref.theta0(r.n, 10).astype(np.float32))
    plain.iterate(10)
    plain_test = plain.rmse()[1]
    plain.close()
    print(f"plain f = 10: test {plain_test:.6f}; ratio {test / plain_test:.4f}")
    assert test <= 0.9 * plain_test
    assert eng.rmse() == (train, test)  # the SSE is summed in a fixed order


def test_mu_is_the_training_mean(alslib, planted):
    from cumf_als_amd import als

    (R, train, _), r = planted
    want = np.float32(R[train].astype(np.float32).astype(np.float64).mean())
    a = float(np.float32(als.bias_mean(r.csr_data).item()))
    b = float(np.float32(als.bias_mean(r.csr_data).item()))
    assert a == b and als.bias_mean(r.csr_data).item() == als.bias_mean(r.csr_data).item()
    assert abs(a - float(want)) <= float(np.spacing(want)), (a, want)
    eng = als.BiasedALSEngine(r, 8, LAM, solver="lu")
    assert eng.mu == a
    eng.close()
    eng = als.BiasedALSEngine(r, 8, LAM, mu=3.25, solver="lu")
    assert eng.mu == 3.25
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. prediction and serving
# ---------------------------------------------------------------------------------------------------------------------
def _chain(q, t):
    """The fp32 fmaf chain in increasing j from +0: each step one fp64 product and sum (exact for fp32 inputs up to the
    final rounding), rounded to fp32."""
    s = np.zeros(q.shape[0], np.float32)
    for j in range(q.shape[1]):
        s = (q[:, j].astype(np.float64) * t[:, j].astype(np.float64) + s.astype(np.float64)).astype(np.float32)
    return s


def test_predict_is_mu_plus_the_chain(alslib, planted, trained):
    (R, _, test), r = planted
    eng, _ = trained
    rows, cols = np.nonzero(test)
    XT, TT = eng.XT.cpu().numpy(), eng.thetaT.cpu().numpy()
    want = np.float32(eng.mu) + _chain(XT[rows], TT[cols])
    got = eng.predict(rows, cols).cpu().numpy()
    assert got.dtype == np.float32 and _same(got, want)
    clipped = eng.predict(rows, cols, clip=(1, 5)).cpu().numpy()
    assert _same(clipped, np.clip(want, np.float32(1), np.float32(5)))
    lo, hi = np.sort(want)[[len(want) // 10, -len(want) // 10]]  # a range that does clip
    tight = eng.predict(rows, cols, clip=(lo, hi)).cpu().numpy()
    assert _same(tight, np.clip(want, lo, hi)) and (tight == lo).sum() > 1 and (tight == hi).sum() > 1
    # the row without ratings predicts mu + c_i
    cols5 = np.arange(r.n)
    got5 = eng.predict(np.full(r.n, 5), cols5).cpu().numpy()
    assert _same(got5, np.float32(eng.mu) + eng.item_bias.cpu().numpy())
    # a NaN row gives NaN, clipped or not
    saved = eng.XT[7].clone()
    eng.XT[7, 0] = float("nan")
    assert np.isnan(eng.predict([7, 7], [0, 1], clip=(1, 5)).cpu().numpy()).all()
    eng.XT[7] = saved


def test_recommend_ranks_by_the_biased_prediction(alslib, planted, trained, reference):
    """recommend(10): mu + score is predict(u, id) bit for bit, and the ids are the reference's top 10 on every row whose
    10th and 11th reference scores differ by more than 1e-4 -- 99.33 % of the rows (tests/test_bias.py asserts >= 95 %)."""
    (R, train, _), r = planted
    eng, _ = trained
    ids, scores = eng.recommend(10)
    torch.cuda.synchronize()
    ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
    assert (ids >= 0).all()
    rows = np.repeat(np.arange(r.m), 10)
    pred = eng.predict(rows, ids.reshape(-1)).cpu().numpy()
    assert _same(np.float32(eng.mu) + scores.reshape(-1), pred)
    assert not train[rows, ids.reshape(-1)].any()  # the training entries are left out
    P = ref.predict(reference["mu"], reference["X"], reference["b"], reference["T"], reference["c"])
    P[train] = -np.inf
    order = np.argsort(-P, axis=1, kind="stable")
    top = np.take_along_axis(P, order[:, :11], axis=1)
    separated = top[:, 9] - top[:, 10] > 1e-4
    print(f"separated rows: {separated.mean():.4f}")
    assert separated.mean() >= 0.95
    wrong = [u for u in np.flatnonzero(separated) if set(ids[u]) != set(order[u, :10])]
    assert not wrong, wrong


def test_inherited_evaluation_ranks_by_the_biased_prediction(alslib, planted, trained):
    """heldout_ranks on the augmented tables: the rank of a held-out entry is the number of unseen items whose chain score
    (the prediction minus mu) is higher, ties to the lower index -- recomputed in numpy for every row."""
    (R, train, test), r = planted
    eng, _ = trained
    ranks, n_eligible, rowptr, colidx = (t.cpu().numpy() for t in eng.heldout_ranks("x"))
    XT, TT = eng.XT.cpu().numpy(), eng.thetaT.cpu().numpy()
    assert int(rowptr[-1]) == int(test.sum())
    for u in range(r.m):
        s = _chain(np.repeat(XT[u:u + 1], r.n, axis=0), TT)
        ok = ~train[u]
        assert n_eligible[u] == ok.sum()
        for e in range(rowptr[u], rowptr[u + 1]):
            t = colidx[e]
            before = ok & ((s > s[t]) | ((s == s[t]) & (np.arange(r.n) < t)))
            assert ranks[e] == before.sum(), (u, t)
    mt = eng.ranking_metrics(10)
    full = eng.full_ranking_metrics(ks=(10,))
    assert mt["queries"] == 299 and 0.0 <= mt["ndcg"] <= 1.0 and 0.0 <= full["auc"] <= 1.0
    th, x = eng.factors()
    assert tuple(th.shape) == (eng.n, 8) and tuple(x.shape) == (eng.m, 8)


@pytest.mark.parametrize("f", [14, 98])
def test_fused_train_sse_is_the_biased_sse(alslib, planted, f):
    """Where the plans deliver it (the wave kernels' routes), the SSE that comes with the Theta half is the biased model's
    train SSE: cumf_bias_sse agrees to 2e-5 relative, the tolerance of test_fused_train_sse_matches_the_rmse_kernel."""
    from cumf_als_amd import als

    _, r = planted
    eng = als.BiasedALSEngine(r, f, LAM, LAM / 4, solver="lu")
    eng.init_factors()
    eng.iterate(2)
    eng.update_x()
    sse = eng.update_theta_with_train_sse()
    want = float(eng.train_sse().item())
    print(f"f = {f}: fused train SSE {None if sse is None else float(sse.item()):}, cumf_bias_sse {want:.9g}")
    assert sse is None or abs(float(sse.item()) - want) <= 2e-5 * want
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(alslib, planted):
    from cumf_als_amd import als

    _, r = planted
    for f in (206, 7, 0):
        with pytest.raises(ValueError):
            als.BiasedALSEngine(r, f, LAM, solver="lu")
    # a plan made at f instead of f + 2: an error, and nothing is launched -- no table or bias changes
    f = 8
    plan = als.Plan(r.csr_indptr, f)
    alslib.cumf_plan_set_gather_rows(plan._h, r.n)
    th0, x0, b0, c0 = _start(r.m, r.n, f + 2)
    g, u = torch.from_numpy(th0).cuda(), torch.from_numpy(x0).cuda()
    gb, ub = torch.from_numpy(c0).cuda(), torch.from_numpy(b0).cuda()
    torch.cuda.synchronize()
    rc = alslib.cumf_bias_update(plan._h, C.c_void_p(r.csr_indices.data_ptr()), C.c_void_p(r.csr_data.data_ptr()),
                                 C.c_void_p(g.data_ptr()), C.c_void_p(gb.data_ptr()), C.c_void_p(u.data_ptr()),
                                 C.c_void_p(ub.data_ptr()), f, 0, 3.5, LAM, LAM, 1, 6, None, None)
    torch.cuda.synchronize()
    assert rc != 0
    assert _same(g.cpu(), th0) and _same(u.cpu(), x0) and _same(gb.cpu(), c0) and _same(ub.cpu(), b0)
    plan.close()
