"""Weighted ALS (include/cumf_weighted_capi.h; als.update_weighted, als.weighted_loss, als.WeightedALSEngine) on the MI355X.

Two reductions are held bit for bit: w = 1, w0 = 0 against als.update_matfree, and w = 1 + 2 |r| on ratings (r > 0) with
w0 = 1 against als.update_implicit(..., solver="cg_matfree") -- there 1 + 2 |r| is an integer <= 11, so w - 1 = alpha |r| and
w (r > 0) = 1 + alpha |r| carry no rounding.  General weights are held to the project's bound for this arithmetic
(tests/test_free_gpu.py above f = 200, test_update_implicit_matfree above f = 128): median, q90 and max of the per-row max-norm
distance to the fp64 oracle.cg (same recurrence, same warm start) on the fp64 systems of tests/weighted_ref.py each within
2 x those of the fp32 oracle.cg + 1e-5 of the scale.  Measured ratios: profiles/weighted/gpu_tests.txt."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import weighted_ref as ref
from tests.test_free_gpu import _exit_case, _seam_rows
from tests.test_implicit_matfree_gpu import _dev, _stats, _table

pytestmark = pytest.mark.gpu

LAM = 0.05
SEAM_COLS = 5000
C_BOUND = 2.0


def _update(rowptr, colidx, val, wgt, Y, x0, w0, reg, iters, cuts=None, chunk=0, route="weighted", alpha=0.0):
    """x0 updated through one plan per row range of `cuts` on the route named; returns x and the last kernel's name."""
    from cumf_als_amd import als

    f = Y.shape[1]
    rows = len(rowptr) - 1
    cuts = [0, rows] if cuts is None else cuts
    cd, vd, Yd, x = _dev(colidx), _dev(np.asarray(val, np.float32)), _dev(Y), _dev(x0.copy())
    wd = None if wgt is None else _dev(np.asarray(wgt, np.float32))
    G = als.implicit_gram(Yd) if (route == "implicit" or w0 > 0) else None
    for a, b in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(rowptr, f, row_begin=a, row_end=b, chunk=chunk)
        if route == "weighted":
            als.update_weighted(plan, cd, vd, wd, Yd, G, x, LAM, w0, reg, iters)
        elif route == "explicit":
            als.update_matfree(plan, cd, vd, Yd, x, LAM, iters)
        else:
            als.update_implicit(plan, cd, vd, Yd, G, x, LAM, alpha, reg, "cg_matfree", iters)
        torch.cuda.synchronize()
        name = als.last_kernel_name()
        plan.close()
    return x.cpu().numpy(), name


def _x0(rows, f, seed=9):
    return (0.05 * np.random.RandomState(seed).standard_normal((rows, f))).astype(np.float32)


def _same(a, b, tag):
    assert np.array_equal(a, b), (tag, np.flatnonzero((a != b).any(1))[:10])


# ---- 1. w = 1, w0 = 0 is the explicit matrix-free route, bit for bit

@pytest.mark.parametrize("f", [10, 66, 190, 254, 318, 382, 446, 510])  # Q = 1 .. 8, the last lane group partly filled
def test_explicit_reduction_is_bit_identical(alslib, f):
    lens, rowptr, colidx, val = _seam_rows()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    ones = np.ones(len(val), np.float32)
    for iters in (1, 6):
        want, _ = _update(rowptr, colidx, val, None, Y, x0, 0.0, "weighted", iters, route="explicit")
        got, name = _update(rowptr, colidx, val, ones, Y, x0, 0.0, "weighted", iters)
        assert "weighted_free_row_kernel" in name, name  # one wave per row: no G, no LDS
        _same(got, want, f"f={f} iters={iters}")
        assert (got[lens == 0] == 0).all()


@pytest.mark.parametrize("f", [258, 64])
def test_explicit_reduction_early_exit(alslib, f):
    """The early-exit case of tests/test_free_gpu.py: rows built to end at steps 1, 2, 3 and never."""
    lens, kinds, rowptr, colidx, val, Y, A64, b64, x0, steps = _exit_case(f)
    ones = np.ones(len(val), np.float32)
    got = {}
    for iters in (1, 2, 3, 6):
        want, _ = _update(rowptr, colidx, val, None, Y, x0, 0.0, "weighted", iters, route="explicit")
        got[iters], _ = _update(rowptr, colidx, val, ones, Y, x0, 0.0, "weighted", iters)
        _same(got[iters], want, f"early exit f={f} iters={iters}")
    for s in (1, 2, 3):  # a row that ended at step s is never touched again
        rows = np.flatnonzero(steps == s)
        assert len(rows) > 0 and np.array_equal(got[6][rows], got[s][rows]), s


def test_explicit_reduction_second_grid_trip(alslib):
    """70 000 rows of one entry at f = 8: more segments than the 16384 workgroups of four waves of one grid hold."""
    f, rows, n_cols = 8, 70_000, 2000
    rng = np.random.RandomState(23)
    rowptr = np.arange(rows + 1, dtype=np.int32)
    colidx = rng.randint(0, n_cols, rows).astype(np.int32)
    val = rng.choice(np.arange(0.5, 5.01, 0.5).astype(np.float32), rows)
    Y, x0 = _table(n_cols, f, 3), _x0(rows, f, 23)
    want, _ = _update(rowptr, colidx, val, None, Y, x0, 0.0, "weighted", 3, route="explicit")
    got, _ = _update(rowptr, colidx, val, np.ones(rows, np.float32), Y, x0, 0.0, "weighted", 3)
    _same(got, want, "70 000 rows")


# ---- 2. w = 1 + alpha |r|, val = (r > 0), w0 = 1 is the implicit matrix-free route, bit for bit

@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("f", [10, 130, 254, 510])
def test_implicit_reduction_is_bit_identical(alslib, f, reg):
    lens, rowptr, colidx, _ = _seam_rows()
    levels = np.arange(0.5, 5.01, 0.5)
    r = np.random.RandomState(31).choice(np.concatenate([-levels, [0.0], levels]).astype(np.float32), int(rowptr[-1]))
    assert (r == 0).any() and (r < 0).any()
    alpha = 2.0
    wgt, pref = (1 + alpha * np.abs(r)).astype(np.float32), (r > 0).astype(np.float32)
    assert np.array_equal(wgt, np.round(wgt)) and wgt.max() <= 11  # integers: w - 1 and w (r > 0) are exact
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    for iters in (1, 3):
        want, _ = _update(rowptr, colidx, r, None, Y, x0, 1.0, reg, iters, route="implicit", alpha=alpha)
        got, name = _update(rowptr, colidx, pref, wgt, Y, x0, 1.0, reg, iters)
        assert "weighted_gram_row_kernel" in name, name
        _same(got, want, f"f={f} {reg} iters={iters}")


# ---- 3. general weights against the fp64 oracle

@functools.lru_cache(maxsize=1)
def _general():
    lens, rowptr, colidx, val = _seam_rows()
    rng = np.random.RandomState(41)
    wgt = rng.uniform(0.5, 4.0, len(val)).astype(np.float32)
    wgt[rng.random_sample(len(val)) < 0.1] = 0.0
    return lens, rowptr, colidx, val, wgt


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("w0", [0.0, 0.3])
@pytest.mark.parametrize("f", [8, 64, 130, 256, 512])
def test_update_weighted_against_the_oracle(oracle, alslib, f, w0, reg):
    lens, rowptr, colidx, val, wgt = _general()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    A64, b64 = ref.systems(rowptr, colidx, val, wgt, Y, LAM, np.float32(w0), reg)  # (w0 as the kernels hold it)
    live = lens > 0
    for iters in (1, 6):
        x64, x32 = np.zeros(x0.shape, np.float64), np.zeros(x0.shape, np.float32)
        x64[live] = oracle.cg(A64[live], x0[live].astype(np.float64), b64[live], f, iters)
        x32[live] = oracle.cg(A64[live].astype(np.float32), x0[live], b64[live].astype(np.float32), f, iters)
        x, name = _update(rowptr, colidx, val, wgt, Y, x0, w0, reg, iters)
        assert ("weighted_gram_row_kernel" if w0 > 0 else "weighted_free_row_kernel") in name, name
        assert (x[~live] == 0).all()
        scale = np.abs(x64).max()
        e_h, e_o = np.abs(x - x64).max(1), np.abs(x32 - x64).max(1)
        s_h, s_o = _stats(e_h[live]), _stats(e_o[live])
        ratio = max(h / o for h, o in zip(s_h, s_o) if o > 0)
        print(f"weighted f={f} w0={w0} {reg} iters={iters}: hip {s_h} oracle32 {s_o} ratio {ratio:.3f} (bound {C_BOUND})")
        for h, o in zip(s_h, s_o):
            assert h <= C_BOUND * o + 1e-5 * scale, (f, w0, reg, iters, s_h, s_o)
        for u in np.flatnonzero(lens >= 2047):  # every long row on its own: one wrong row cannot hide in the statistics
            assert e_h[u] <= C_BOUND * s_o[2] + 1e-5 * scale, (f, w0, reg, iters, int(u), int(lens[u]), float(e_h[u]), s_o)


# ---- 4. determinism and plan independence

def test_weighted_is_deterministic_and_plan_independent(alslib):
    f, w0 = 254, 0.3
    lens, rowptr, colidx, val, wgt = _general()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    x1, _ = _update(rowptr, colidx, val, wgt, Y, x0, w0, "weighted", 6)
    x2, _ = _update(rowptr, colidx, val, wgt, Y, x0, w0, "weighted", 6)
    _same(x2, x1, "second run")
    xc, _ = _update(rowptr, colidx, val, wgt, Y, x0, w0, "weighted", 6, cuts=[0, 7, 30, 45])
    _same(xc, x1, "row ranges")
    xc, _ = _update(rowptr, colidx, val, wgt, Y, x0, w0, "weighted", 6, chunk=64)
    _same(xc, x1, "chunk 64")


# ---- 5. refusals

def test_update_weighted_refusals(alslib, capfd):
    from cumf_als_amd import als

    rowptr = np.array([0, 2, 3], np.int32)
    colidx, val = _dev(np.array([0, 1, 1], np.int32)), _dev(np.array([1.0, 2.0, 3.0], np.float32))
    wgt = _dev(np.array([1.0, 0.5, 2.0], np.float32))
    f = 64
    table = _dev(_table(2, f, 1))
    start = _table(2, f, 2)
    x = _dev(start.copy())
    G = als.implicit_gram(table)
    plan = als.Plan(rowptr, f)
    with pytest.raises(ValueError):
        als.update_weighted(plan, colidx, val, wgt, table, G, x, LAM, w0=-1.0)
    with pytest.raises(ValueError):
        als.update_weighted(plan, colidx, val, wgt, table, None, x, LAM, w0=0.5)
    # ... and by the library itself
    ptr = lambda t: t.data_ptr()  # noqa: E731
    for w0, g in ((-1.0, ptr(G)), (float("nan"), ptr(G)), (0.5, None)):
        capfd.readouterr()
        assert alslib.cumf_als_update_weighted(plan._h, ptr(colidx), ptr(val), ptr(wgt), ptr(table), g, ptr(x), LAM, w0, 0, 6,
                                               None) == 1, w0
        assert "cumf_als_update_weighted" in capfd.readouterr().err
    assert alslib.cumf_als_update_weighted(plan._h, ptr(colidx), ptr(val), ptr(wgt), ptr(table), ptr(G), ptr(x), LAM, 0.5, 2, 6,
                                           None) == 1  # an unknown reg mode
    plan.close()
    # f = 6: a plan of it exists (cumf_plan_create takes any even f up to 512), so the f check of the route itself is what
    # refuses -- the wrapper's, and the library's behind it
    plan6 = als.Plan(rowptr, 6)
    table6, x6 = _dev(_table(2, 6, 1)), _dev(_table(2, 6, 2))
    start6 = x6.cpu().numpy().copy()
    with pytest.raises(ValueError):
        als.update_weighted(plan6, colidx, val, wgt, table6, None, x6, LAM)
    capfd.readouterr()
    assert alslib.cumf_als_update_weighted(plan6._h, ptr(colidx), ptr(val), ptr(wgt), ptr(table6), None, ptr(x6), LAM, 0.0, 0, 6,
                                           None) == 1
    assert "even 8 <= f <= 512 (got 6)" in capfd.readouterr().err
    plan6.close()
    torch.cuda.synchronize()
    assert np.array_equal(x6.cpu().numpy(), start6)
    for bad in (9, 514):  # no plan of such an f exists: cumf_plan_create refuses it before the route is asked
        with pytest.raises((ValueError, RuntimeError)):
            als.update_weighted(als.Plan(rowptr, bad), colidx, val, wgt, table, None, x, LAM)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), start)  # every refusal left `update` as it was


# ---- 6. the engine

@pytest.fixture(scope="module")
def engine_data():
    from cumf_als_amd import datagen

    return datagen.synth_ratings(300, 200, 6000, 600, seed=5).to("cuda")


def _weights(r, seed=13):
    w = np.random.RandomState(seed).uniform(0.25, 4.0, r.nnz).astype(np.float32)
    w[::17] = 0.0
    return w


@pytest.mark.parametrize("f", [16, 258])
def test_engine_is_the_hand_driven_sequence(alslib, engine_data, f):
    from cumf_als_amd import als

    r, w0 = engine_data, 0.3
    w = _weights(r)
    d = r.numpy()
    # the CSC weights by an independent route: numpy's lexsort by (column, row) of the CSR entries
    order = np.lexsort((d["coo_row"], d["csr_indices"]))
    assert np.array_equal(d["coo_row"][order], d["csc_indices"]) and np.array_equal(d["csr_data"][order], d["csc_data"])
    w_csc = _dev(w[order])
    eng = als.WeightedALSEngine(r, _dev(w), f, LAM, w0=w0)
    eng.init_factors(seed=1)
    X, T = eng.XT.clone(), eng.thetaT.clone()
    eng.iterate(2)
    px, pt = als.Plan(d["csr_indptr"], f), als.Plan(d["csc_indptr"], f)
    for _ in range(2):
        als.update_weighted(px, r.csr_indices, r.csr_data, eng.w_csr, T, als.implicit_gram(T), X, LAM, w0)
        als.update_weighted(pt, r.csc_indices, r.csc_data, w_csc, X, als.implicit_gram(X), T, LAM, w0)
    torch.cuda.synchronize()
    assert torch.equal(eng.XT, X) and torch.equal(eng.thetaT, T)
    assert torch.equal(eng.w_csc, w_csc)
    px.close()
    pt.close()
    # the objective: the kernel, the same identity in numpy, and brute force over all m x n entries
    Xh, Th = X.cpu().numpy(), T.cpu().numpy()
    for reg in ("weighted", "plain"):
        got = float(als.weighted_loss(eng.csr_rowptr, r.csr_indices, r.csr_data, eng.w_csr, X, T, LAM, w0, reg).item())
        sparse = ref.sparse_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], w, Xh, Th, LAM, np.float32(w0), reg)
        dense = ref.dense_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], w, Xh, Th, LAM, np.float32(w0), reg)
        print(f"weighted loss f={f} {reg}: hip {got!r} sparse {sparse!r} dense {dense!r}")
        assert abs(got - sparse) <= 1e-6 * abs(sparse) and abs(got - dense) <= 1e-6 * abs(dense), (reg, got, sparse, dense)
    assert eng.loss() == float(als.weighted_loss(eng.csr_rowptr, r.csr_indices, r.csr_data, eng.w_csr, X, T, LAM, w0).item())
    # batches
    eng3 = als.WeightedALSEngine(r, _dev(w), f, LAM, w0=w0, x_batch=3, theta_batch=2)
    eng3.init_factors(seed=1)
    eng3.iterate(2)
    assert torch.equal(eng3.XT, eng.XT) and torch.equal(eng3.thetaT, eng.thetaT)
    ids, _ = eng.recommend(5)
    ids = ids.cpu().numpy()
    assert ids.shape == (r.m, 5) and (ids >= 0).all() and (ids < r.n).all()
    eng.close()
    eng3.close()


@pytest.mark.parametrize("w0", [0.0, 0.3])
@pytest.mark.parametrize("f", [16, 258])
def test_engine_loss_is_non_increasing(alslib, engine_data, f, w0):
    from cumf_als_amd import als

    r = engine_data
    e = als.WeightedALSEngine(r, _dev(_weights(r)), f, LAM, w0=w0)
    e.init_factors(seed=1)
    e.update_x()
    prev = e.loss()
    losses = [prev]
    for _ in range(3):
        for half in (e.update_theta, e.update_x):
            half()
            cur = e.loss()
            losses.append(cur)
            assert cur <= prev + 1e-6 * abs(prev), (f, w0, losses)  # the slack of the implicit engine's test
            prev = cur
    print(f"weighted engine f={f} w0={w0}: loss after each half-iteration {[round(v, 4) for v in losses]}")
    assert losses[-1] < losses[0]
    e.close()


@pytest.mark.parametrize("f", [16, 258])
def test_engine_reductions_are_bit_identical(alslib, engine_data, f):
    """WeightedALSEngine(w = 1, w0 = 0) is ALSEngine(solver="cg_matfree"), and the alpha = 2 construction is
    ImplicitALSEngine(solver="cg_matfree"), bit for bit after two iterations."""
    from cumf_als_amd import als

    r = engine_data
    want = als.ALSEngine(r, f, LAM, solver="cg_matfree", cg_iters=6)
    got = als.WeightedALSEngine(r, torch.ones_like(r.csr_data), f, LAM, w0=0.0, cg_iters=6)
    assert got.G is None  # no Gram at w0 = 0
    for e in (want, got):
        e.init_factors(seed=1)
        e.iterate(2)
    assert torch.equal(got.XT, want.XT) and torch.equal(got.thetaT, want.thetaT)
    # ratings 1 .. 5 -> strengths -1 .. 3 (integers, with negatives and stored zeros)
    alpha = 2.0
    strength = dataclasses.replace(r, csr_data=r.csr_data - 2.0, csc_data=r.csc_data - 2.0)
    pref = dataclasses.replace(r, csr_data=(strength.csr_data > 0).float(), csc_data=(strength.csc_data > 0).float())
    assert bool((strength.csr_data == 0).any()) and bool((strength.csr_data < 0).any())
    for reg in ("weighted", "plain"):
        want_i = als.ImplicitALSEngine(strength, f, LAM, alpha, solver="cg_matfree", cg_iters=3, reg=reg)
        got_i = als.WeightedALSEngine(pref, 1 + alpha * strength.csr_data.abs(), f, LAM, w0=1.0, reg=reg, cg_iters=3)
        for e in (want_i, got_i):
            e.init_factors(seed=1)
            e.iterate(2)
        assert torch.equal(got_i.XT, want_i.XT) and torch.equal(got_i.thetaT, want_i.thetaT), reg
        assert abs(got_i.loss() - want_i.loss()) <= 1e-9 * abs(want_i.loss())  # the same objective, two fp64 evaluations
    for e in (want, got, want_i, got_i):
        e.close()


def test_engine_refuses_bad_weights(alslib, engine_data):
    from cumf_als_amd import als

    r = engine_data
    w = torch.ones_like(r.csr_data)
    for bad in (-1.0, float("nan"), float("inf")):
        wb = w.clone()
        wb[5] = bad
        with pytest.raises(ValueError):
            als.WeightedALSEngine(r, wb, 16, LAM)
    with pytest.raises(ValueError):
        als.WeightedALSEngine(r, w, 514, LAM)
    with pytest.raises(ValueError):
        als.WeightedALSEngine(r, w, 16, LAM, w0=-0.5)
    # a dataset whose CSC arrays are not its CSR entries in (column, row) order
    broken = dataclasses.replace(r, csc_data=r.csc_data.flip(0).contiguous())
    with pytest.raises(ValueError):
        als.WeightedALSEngine(broken, w, 16, LAM)
