"""Weighted ALS with rank-one weights a_u c_i on the unstored entries (include/cumf_weighted_capi.h; als.weighted_gram,
als.update_weighted_rank1, als.weighted_rank1_loss, als.WeightedALSEngine(unobserved=...)) on the MI355X.

Two reductions are held bit for bit: weighted_gram with row_w = 1 against als.implicit_gram (1 y is y), and gather_w0 = 1,
own_w0 = w0 against als.update_weighted (fma(-w0, 1, w) is w - w0 rounded once; the per-row scale of G v is the scalar one).
General weights are held to the bound of tests/test_weighted_gpu.py for this arithmetic: median, q90 and max of the per-row
max-norm distance to the fp64 oracle.cg (same recurrence, same warm start) on the fp64 systems of tests/weighted_rank1_ref.py
each within 2 x those of the fp32 oracle.cg + 1e-5 of the scale.  Measured ratios: profiles/weighted_rank1/gpu_tests.txt."""
import functools

import numpy as np
import pytest
import torch

from tests import weighted_rank1_ref as ref
from tests.test_free_gpu import _exit_case, _seam_rows
from tests.test_implicit_matfree_gpu import _dev, _stats, _table
from tests.test_weighted_gpu import C_BOUND, LAM, SEAM_COLS, _general, _same, _x0
from tests.test_weighted_gpu import _update as _update_w0

pytestmark = pytest.mark.gpu

ROW_KERNEL = "weighted_rank1_row_kernel"


def _update(rowptr, colidx, val, wgt, Y, x0, own, gather, reg, iters, cuts=None, chunk=0):
    """x0 updated by update_weighted_rank1 through one plan per row range of `cuts`; returns x and the last kernel's name."""
    from cumf_als_amd import als

    f = Y.shape[1]
    rows = len(rowptr) - 1
    cuts = [0, rows] if cuts is None else cuts
    cd, vd, wd, Yd, x = _dev(colidx), _dev(np.asarray(val, np.float32)), _dev(np.asarray(wgt, np.float32)), _dev(Y), _dev(x0.copy())
    od, gd = _dev(np.asarray(own, np.float32)), _dev(np.asarray(gather, np.float32))
    G = als.weighted_gram(Yd, gd)
    for a, b in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(rowptr, f, row_begin=a, row_end=b, chunk=chunk)
        als.update_weighted_rank1(plan, cd, vd, wd, Yd, G, od, gd, x, LAM, reg, iters)
        torch.cuda.synchronize()
        name = als.last_kernel_name()
        plan.close()
    return x.cpu().numpy(), name


def _tenth_zero(rng, lo, hi, n):
    v = rng.uniform(lo, hi, n).astype(np.float32)
    v[rng.choice(n, max(1, n // 10), replace=False)] = 0.0
    return v


# ---- 1. the weighted Gram

@pytest.mark.parametrize("f", [8, 10, 100, 128, 130, 254, 512])
def test_weighted_gram(alslib, f):
    from cumf_als_amd import als

    for rows in (1, 1000, 3001, 9000):  # 3001: past the 1024-row slab, no multiple of the 32-row stage; 9000: past 2 x 4096
        Y = _table(rows, f, rows + f)
        Yd = _dev(Y)
        ones = torch.ones(rows, dtype=torch.float32, device="cuda")
        assert torch.equal(als.weighted_gram(Yd, ones), als.implicit_gram(Yd)), (f, rows)
        c = _tenth_zero(np.random.RandomState(rows + 7 * f), 0.0, 3.0, rows)
        g, g2 = als.weighted_gram(Yd, _dev(c)).cpu().numpy(), als.weighted_gram(Yd, _dev(c)).cpu().numpy()
        Y64, c64 = Y.astype(np.float64), c.astype(np.float64)
        err = np.abs(g - (Y64 * c64[:, None]).T @ Y64)
        assert (err <= 1e-5 * ((np.abs(Y64) * c64[:, None]).T @ np.abs(Y64))).all(), (f, rows, err.max())
        assert np.array_equal(g, g2) and np.array_equal(g, g.T), (f, rows)


# ---- 2. gather_w0 = 1, own_w0 = w0 is update_weighted, bit for bit

W0 = np.float32(0.3)


def _reduction(f, reg, iters_list):
    lens, rowptr, colidx, val, wgt = _general()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    own, gather = np.full(len(lens), W0, np.float32), np.ones(SEAM_COLS, np.float32)
    for iters in iters_list:
        want, _ = _update_w0(rowptr, colidx, val, wgt, Y, x0, float(W0), reg, iters)
        got, name = _update(rowptr, colidx, val, wgt, Y, x0, own, gather, reg, iters)
        assert ROW_KERNEL in name, name
        _same(got, want, f"f={f} {reg} iters={iters}")
        assert (got[lens == 0] == 0).all()


@pytest.mark.parametrize("f", [10, 66, 190, 254, 318, 382, 446, 510])  # Q = 1 .. 8, the last lane group partly filled
def test_scalar_reduction_is_bit_identical(alslib, f):
    _reduction(f, "weighted", (1, 6))


@pytest.mark.parametrize("f", [10, 254])
def test_scalar_reduction_plain_reg(alslib, f):
    _reduction(f, "plain", (1, 6))


@pytest.mark.parametrize("f", [258, 64])
def test_scalar_reduction_early_exit(alslib, f):
    """The early-exit case of tests/test_free_gpu.py.  At own_w0 = 0.3 every step count returns update_weighted's bits; at
    own_w0 = 0 the systems are the explicit ones the case was built on, whose rows end at steps 1, 2, 3 and never: a row
    that ended is never touched again."""
    lens, kinds, rowptr, colidx, val, Y, A64, b64, x0, steps = _exit_case(f)
    ones = np.ones(len(val), np.float32)
    gather = np.ones(len(Y), np.float32)
    got = {}
    for iters in (1, 2, 3, 6):
        want, _ = _update_w0(rowptr, colidx, val, ones, Y, x0, float(W0), "weighted", iters)
        g, name = _update(rowptr, colidx, val, ones, Y, x0, np.full(len(lens), W0, np.float32), gather, "weighted", iters)
        assert ROW_KERNEL in name, name
        _same(g, want, f"early exit f={f} iters={iters}")
        got[iters], _ = _update(rowptr, colidx, val, ones, Y, x0, np.zeros(len(lens), np.float32), gather, "weighted", iters)
    for s in (1, 2, 3):
        rows = np.flatnonzero(steps == s)
        assert len(rows) > 0 and np.array_equal(got[6][rows], got[s][rows]), s


# ---- 3. general rank-one weights against the fp64 oracle

@functools.lru_cache(maxsize=1)
def _rank1():
    """a over the 45 seam rows from uniform [0, 1], c over the 5000 columns from uniform [0, 2], a tenth of each 0: the two
    lengths differ, so a swapped own / gather index reads other weights (or past the 45)."""
    lens = _general()[0]
    rng = np.random.RandomState(43)
    return _tenth_zero(rng, 0.0, 1.0, len(lens)), _tenth_zero(rng, 0.0, 2.0, SEAM_COLS)


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("f", [8, 64, 130, 256, 512])
def test_update_weighted_rank1_against_the_oracle(oracle, alslib, f, reg):
    lens, rowptr, colidx, val, wgt = _general()
    a, c = _rank1()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    A64, b64 = ref.systems(rowptr, colidx, val, wgt, Y, LAM, a, c, reg)  # (a, c as the kernels hold them: fp32 values)
    live = lens > 0
    for iters in (1, 6):
        x64, x32 = np.zeros(x0.shape, np.float64), np.zeros(x0.shape, np.float32)
        x64[live] = oracle.cg(A64[live], x0[live].astype(np.float64), b64[live], f, iters)
        x32[live] = oracle.cg(A64[live].astype(np.float32), x0[live], b64[live].astype(np.float32), f, iters)
        x, name = _update(rowptr, colidx, val, wgt, Y, x0, a, c, reg, iters)
        assert ROW_KERNEL in name, name
        assert (x[~live] == 0).all()
        scale = np.abs(x64).max()
        e_h, e_o = np.abs(x - x64).max(1), np.abs(x32 - x64).max(1)
        s_h, s_o = _stats(e_h[live]), _stats(e_o[live])
        ratio = max(h / o for h, o in zip(s_h, s_o) if o > 0)
        print(f"weighted rank1 f={f} {reg} iters={iters}: hip {s_h} oracle32 {s_o} ratio {ratio:.3f} (bound {C_BOUND})")
        for h, o in zip(s_h, s_o):
            assert h <= C_BOUND * o + 1e-5 * scale, (f, reg, iters, s_h, s_o)
        for u in np.flatnonzero(lens >= 2047):  # every long row on its own: one wrong row cannot hide in the statistics
            assert e_h[u] <= C_BOUND * s_o[2] + 1e-5 * scale, (f, reg, iters, int(u), int(lens[u]), float(e_h[u]), s_o)


# ---- 4. determinism and plan independence

def test_rank1_is_deterministic_and_plan_independent(alslib):
    f = 254
    lens, rowptr, colidx, val, wgt = _general()
    a, c = _rank1()
    Y, x0 = _table(SEAM_COLS, f, 3), _x0(len(lens), f)
    x1, _ = _update(rowptr, colidx, val, wgt, Y, x0, a, c, "weighted", 6)
    x2, _ = _update(rowptr, colidx, val, wgt, Y, x0, a, c, "weighted", 6)
    _same(x2, x1, "second run")
    xc, _ = _update(rowptr, colidx, val, wgt, Y, x0, a, c, "weighted", 6, cuts=[0, 7, 30, 45])  # own_w0 by absolute row
    _same(xc, x1, "row ranges")
    xc, _ = _update(rowptr, colidx, val, wgt, Y, x0, a, c, "weighted", 6, chunk=64)
    _same(xc, x1, "chunk 64")


# ---- 5. the objective

@pytest.fixture(scope="module")
def small_data():
    from cumf_als_amd import datagen

    return datagen.synth_ratings(60, 40, 600, 60, seed=5).to("cuda")


def _small_weights(r, seed=13):
    rng = np.random.RandomState(seed)
    w = rng.uniform(0.25, 4.0, r.nnz).astype(np.float32)
    w[::17] = 0.0
    return w, _tenth_zero(rng, 0.0, 1.0, r.m), _tenth_zero(rng, 0.0, 2.0, r.n)


@pytest.mark.parametrize("f", [16, 258])
def test_rank1_loss_is_the_dense_loss(alslib, small_data, f):
    from cumf_als_amd import als

    r = small_data
    d = r.numpy()
    w, a, c = _small_weights(r)
    rng = np.random.RandomState(f)
    X, T = (0.3 * rng.standard_normal((r.m, f))).astype(np.float32), (0.3 * rng.standard_normal((r.n, f))).astype(np.float32)
    rowptr = r.csr_indptr.to(device="cuda", dtype=torch.int32)
    for reg in ("weighted", "plain"):
        got = float(als.weighted_rank1_loss(rowptr, r.csr_indices, r.csr_data, _dev(w), _dev(X), _dev(T), _dev(a), _dev(c), LAM,
                                            reg).item())
        dense = ref.dense_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], w, X, T, LAM, a, c, reg)
        print(f"weighted rank1 loss f={f} {reg}: hip {got!r} dense {dense!r} rel {abs(got - dense) / abs(dense):.2e}")
        assert abs(got - dense) <= 1e-6 * abs(dense), (reg, got, dense)


@pytest.mark.parametrize("f", [16, 258])
def test_engine_loss_is_non_increasing(alslib, small_data, f):
    from cumf_als_amd import als

    r = small_data
    w, a, c = _small_weights(r)
    e = als.WeightedALSEngine(r, _dev(w), f, LAM, unobserved=(_dev(a), _dev(c)))
    e.init_factors(seed=1)
    e.update_x()
    prev = e.loss()
    losses = [prev]
    for _ in range(3):
        for half in (e.update_theta, e.update_x):
            half()
            cur = e.loss()
            losses.append(cur)
            assert cur <= prev + 1e-6 * abs(prev), (f, losses)
            prev = cur
    print(f"weighted rank1 engine f={f}: loss after each half-iteration {[round(v, 4) for v in losses]}")
    assert losses[-1] < losses[0]
    # the engine's objective is the function's
    d = r.numpy()
    dense = ref.dense_loss(d["csr_indptr"], d["csr_indices"], d["csr_data"], w, e.XT.cpu().numpy(), e.thetaT.cpu().numpy(), LAM,
                           a, c)
    assert abs(losses[-1] - dense) <= 1e-6 * abs(dense), (losses[-1], dense)
    e.close()


# ---- 6. the engine

@pytest.mark.parametrize("f", [16, 130])
def test_engine_reduction_is_bit_identical(alslib, small_data, f):
    """unobserved=(full(m, 0.3), ones(n)) trains what w0 = 0.3 does, bit for bit, on both sides: the engine hands each
    half-iteration the pair with the largest gather weight moved into the own vector, so the Theta side too runs own = 0.3,
    gather = 1 (with gather = 0.3 its Gram X^T diag(0.3) X would differ from 0.3 X^T X by roundings, and a row whose r.r
    then crosses 1e-4 a step earlier by 1e-2)."""
    from cumf_als_amd import als

    r = small_data
    w = _dev(_small_weights(r)[0])
    want = als.WeightedALSEngine(r, w, f, LAM, w0=0.3)
    got = als.WeightedALSEngine(r, w, f, LAM, unobserved=(torch.full((r.m,), 0.3, dtype=torch.float32, device="cuda"),
                                                          torch.ones(r.n, dtype=torch.float32, device="cuda")))
    for e in (want, got):
        e.init_factors(seed=1)
        e.iterate(2)
    assert torch.equal(got.XT, want.XT) and torch.equal(got.thetaT, want.thetaT)
    # the same objective; the rank-one one sums fp32 partials of X^T diag(0.3) X, the scalar one of X^T X: the bound of 5.
    assert abs(got.loss() - want.loss()) <= 1e-6 * abs(want.loss())
    want.close()
    got.close()


def test_engine_refuses_bad_unobserved_weights(alslib, small_data):
    from cumf_als_amd import als

    r = small_data
    w = torch.ones_like(r.csr_data)
    a, c = torch.ones(r.m, dtype=torch.float32, device="cuda"), torch.ones(r.n, dtype=torch.float32, device="cuda")
    als.WeightedALSEngine(r, w, 16, LAM, unobserved=(a, c)).close()
    with pytest.raises(ValueError):
        als.WeightedALSEngine(r, w, 16, LAM, w0=0.5, unobserved=(a, c))
    for bad in (-1.0, float("nan"), float("inf")):
        for which in (0, 1):
            pair = [a.clone(), c.clone()]
            pair[which][3] = bad
            with pytest.raises(ValueError):
                als.WeightedALSEngine(r, w, 16, LAM, unobserved=tuple(pair))
    with pytest.raises(TypeError):  # the two lengths swapped
        als.WeightedALSEngine(r, w, 16, LAM, unobserved=(c, a))


# ---- 7. refusals of the half-iteration that need a plan

def test_update_weighted_rank1_refusals(alslib, capfd):
    from cumf_als_amd import als

    rowptr = np.array([0, 2, 3], np.int32)
    colidx, val = _dev(np.array([0, 1, 1], np.int32)), _dev(np.array([1.0, 2.0, 3.0], np.float32))
    wgt, own, gat = _dev(np.array([1.0, 0.5, 2.0], np.float32)), _dev(np.array([0.5, 0.25], np.float32)), _dev(np.ones(2, np.float32))
    ptr = lambda t: t.data_ptr()  # noqa: E731
    f = 64
    table, start = _dev(_table(2, f, 1)), _table(2, f, 2)
    x = _dev(start.copy())
    G = als.weighted_gram(table, gat)
    plan = als.Plan(rowptr, f)
    args = [plan._h, ptr(colidx), ptr(val), ptr(wgt), ptr(table), ptr(G), ptr(own), ptr(gat), ptr(x)]
    for k in range(len(args)):  # each pointer in turn NULL: G, own_w0 and gather_w0 are required too
        capfd.readouterr()
        bad = list(args)
        bad[k] = None
        assert alslib.cumf_als_update_weighted_rank1(*bad, LAM, 0, 6, None) == 1, k
        assert "cumf_als_update_weighted_rank1" in capfd.readouterr().err
    assert alslib.cumf_als_update_weighted_rank1(*args, LAM, 2, 6, None) == 1  # an unknown reg mode
    for none in ("G", "own_w0", "gather_w0"):
        kw = dict(G=G, own_w0=own, gather_w0=gat)
        kw[none] = None
        with pytest.raises(ValueError):
            als.update_weighted_rank1(plan, colidx, val, wgt, table, kw["G"], kw["own_w0"], kw["gather_w0"], x, LAM)
    with pytest.raises(TypeError):  # own_w0 and gather_w0 of the wrong lengths
        als.update_weighted_rank1(plan, colidx, val, wgt, table, G, _dev(np.ones(3, np.float32)), gat, x, LAM)
    plan.close()
    plan6 = als.Plan(rowptr, 6)  # a plan of f = 6 exists: the route's own f check refuses
    table6, x6 = _dev(_table(2, 6, 1)), _dev(_table(2, 6, 2))
    capfd.readouterr()
    assert alslib.cumf_als_update_weighted_rank1(plan6._h, ptr(colidx), ptr(val), ptr(wgt), ptr(table6), ptr(G), ptr(own), ptr(gat),
                                                 ptr(x6), LAM, 0, 6, None) == 1
    assert "even 8 <= f <= 512 (got 6)" in capfd.readouterr().err
    with pytest.raises(ValueError):
        als.update_weighted_rank1(plan6, colidx, val, wgt, table6, G, own, gat, x6, LAM)
    plan6.close()
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy(), start)  # every refusal left `update` as it was
