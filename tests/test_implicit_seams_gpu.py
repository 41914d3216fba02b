"""The materialised implicit routes ("lu", "cg"; als_implicit.hip, als_implicit.cpp) at the seams tests/test_implicit_gpu.py
leaves out: every tile count FT = ceil(f / 16) = 1..8 of implicit_hermitian_kernel (both output modes) and of
implicit_gram_partial_kernel at its narrowest and at its full width, rows of two chunks, last chunks of one entry and several
chunked rows in one plan, every row length 0..33 of implicit_short_cg_kernel with the f = 64 / 66 lane seam and its grid-stride
second pass, plans over a sub-range of mixed rows on both routes, the degenerate plans, and the objective below one row per wave
and through the wide Gram.  Tiny shapes: a gather table of 300 rows, tens of rows per plan.  References, bounds and helpers
are those of tests/test_implicit_gpu.py and tests/test_implicit_matfree_seams_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import implicit_ref as ref
from tests.test_implicit_gpu import _dev, _table
from tests.test_implicit_matfree_gpu import _stats
from tests.test_implicit_matfree_seams_gpu import CG_EXIT, LAM, VALUES, _cg_rs, _csr, _oracles

pytestmark = pytest.mark.gpu

N_TABLE = 300  # gather table rows
MODES = ((1.0, "weighted"), (40.0, "plain"))  # (alpha, reg)
# the narrowest and the full width of every tile count FT = 1..8 (f even, at least 8)
F_EDGES = [8, 16, 18, 32, 34, 48, 50, 64, 66, 80, 82, 96, 98, 112, 114, 128]
assert F_EDGES == sorted(f for FT in range(1, 9) for f in (max(8, 16 * (FT - 1) + 2), 16 * FT))
assert sorted({-(-f // 16) for f in F_EDGES}) == list(range(1, 9))


def _x0(rows, f, seed=9):
    return (0.05 * np.random.RandomState(seed).standard_normal((rows, f))).astype(np.float32)


def _update(rowptr, colidx, val, Y, x0, alpha, reg, solver, iters, chunk=0, row_begin=0, row_end=None):
    """x0 updated through one plan of rows [row_begin, row_end); returns x and the last kernel's name."""
    from cumf_als_amd import als

    plan = als.Plan(rowptr, Y.shape[1], row_begin=row_begin, row_end=row_end, chunk=chunk)
    Yg = _dev(Y)
    x = _dev(x0.copy())
    als.update_implicit(plan, _dev(colidx), _dev(val), Yg, als.implicit_gram(Yg), x, LAM, alpha, reg, solver, iters)
    torch.cuda.synchronize()
    name = als.last_kernel_name()
    plan.close()
    return x.cpu().numpy(), name


def _check_rows(x, x64, x32, lens, tag):
    """Every non-empty row on its own: max-norm distance to the fp64 oracle.cg within 1.05 x the largest row error of the fp32
    oracle.cg + 1e-5 of the scale (the per-row form of test_implicit_matfree_seams_gpu._check); empty rows exactly 0."""
    empty = lens == 0
    assert (x[empty] == 0).all(), tag
    if empty.all():
        return
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1)[~empty], np.abs(x32 - x64).max(1)[~empty]
    print(f"implicit seams {tag}: hip max {e_h.max():.3e} oracle32 max {e_o.max():.3e} ratio {e_h.max() / e_o.max():.3f}")
    bad = np.flatnonzero(e_h > 1.05 * e_o.max() + 1e-5 * scale)
    assert len(bad) == 0, (tag, np.flatnonzero(~empty)[bad], e_h[bad], e_o.max(), scale)


def _check_dist(x, x64, x32, lens, tag):
    """The rule of test_update_implicit_cg: median / q90 / max of the per-row max-norm distance to the fp64 oracle.cg within
    1.05 x those of the fp32 oracle.cg + 1e-5 of the scale; empty rows exactly 0."""
    empty = lens == 0
    assert (x[empty] == 0).all(), tag
    scale = np.abs(x64).max()
    s_h, s_o = _stats(np.abs(x - x64).max(1)[~empty]), _stats(np.abs(x32 - x64).max(1)[~empty])
    print(f"implicit seams {tag}: hip {s_h} oracle32 {s_o} ratio {max(h / o for h, o in zip(s_h, s_o)):.3f}")
    for h, o in zip(s_h, s_o):
        assert h <= 1.05 * o + 1e-5 * scale, (tag, s_h, s_o)


def _check_lu(x, A64, b64, oracle, lens, f, tag):
    """The bound of test_update_implicit_lu: per row within 2 x the fp32 oracle LU's distance from fp64 + 1e-5 of the scale."""
    empty = lens == 0
    assert (x[empty] == 0).all(), tag
    if empty.all():
        return
    x64 = np.linalg.solve(A64, b64[..., None])[..., 0]
    x32 = oracle.lu(A64.astype(np.float32), b64.astype(np.float32), f)
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1)[~empty], np.abs(x32 - x64).max(1)[~empty]
    print(f"implicit seams {tag}: hip max {e_h.max():.3e} oracle32 max {e_o.max():.3e} ratio {e_h.max() / e_o.max():.3f}")
    bad = np.flatnonzero(e_h > 2 * e_o + 1e-5 * scale)
    assert len(bad) == 0, (tag, np.flatnonzero(~empty)[bad], e_h[bad], e_o[bad], scale)


def _assert_exit_clear(A64, b64, x0, lens, tag):
    """The condition under which a 3-step run may be compared with the oracle: in fp64, no row's r.r after step 1 or 2 (the
    two that the exit test can act on) lies within a factor of 4 of CG_EXIT, so fp32 ends every row where fp64 does."""
    for u in np.flatnonzero(lens > 0):
        rs, _ = _cg_rs(A64[u], x0[u], b64[u], 3)
        assert all(v < CG_EXIT / 4 or v > CG_EXIT * 4 for v in rs[1:3]), (tag, int(u), int(lens[u]), rs)


# ---- 1. systems at every tile count

# long and short rows interleaved in row index; 33 and 65 twice
SEAM_LENS = np.array([33, 0, 64, 1, 129, 31, 63, 32, 96, 5, 65, 2, 97, 20, 33, 11, 65, 17, 9])
assert set(SEAM_LENS) >= {0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 129}


@functools.lru_cache(maxsize=1)
def _seam_rows():
    return _csr(list(SEAM_LENS), N_TABLE, np.random.RandomState(31))


@pytest.mark.parametrize("f", F_EDGES)
def test_systems_at_every_tile_count(alslib, f):
    """implicit_hermitian_kernel<FT> and <kImpPacked + FT> with implicit_slot_reduce(_packed)_kernel and implicit_finish_kernel
    at chunk = 32 and 64: rows of one stage, of two chunks, of a last chunk of one entry, several chunked rows in one plan.

    Symmetry.  Entries (i, j) and (j, i) that lie in DIFFERENT 16-blocks are bit-identical: the kernel computes the upper tile
    and stores each value twice (the slot reduce and G keep that).  Inside a diagonal tile the two halves are computed
    independently, fl(w y_i) y_j against fl(w y_j) y_i, and agree only to rounding: they are held to the tolerance of the
    systems and NOT to equal bits.  Full bitwise symmetry is not a property of this kernel.

    Packed mode.  In plain mode a whole row's upper triangle of implicit_finish(partial, G, lambda) has the bits of
    get_hermitian_implicit: the item code is the same and the two fp32 additions (+ G, + lambda) come in the same order.  In
    weighted mode, and for chunked rows, the additions are ordered differently and only the tolerance holds."""
    from cumf_als_amd import als

    lens = SEAM_LENS
    rowptr, colidx, val = _seam_rows()
    Y = _table(N_TABLE, f, 3)
    cg, vg, Yg = _dev(colidx), _dev(val), _dev(Y)
    G = als.implicit_gram(Yg)
    blk = np.arange(f) // 16
    off = blk[:, None] != blk[None, :]
    iu = np.triu_indices(f)
    refs = {}
    for alpha, reg in MODES:
        A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
        Aabs, _ = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg, absolute=True)
        refs[alpha, reg] = A64, b64, Aabs, ref.rhs_scale(rowptr, colidx, val, Y, alpha)
    worst = 0.0
    for chunk in (32, 64):
        plan = als.Plan(rowptr, f, chunk=chunk)
        multi = lens > chunk
        assert plan.chunk == chunk and plan.n_multi_rows == multi.sum() and plan.n_multi_rows >= (4 if chunk == 32 else 2)
        assert plan.n_slots == sum(-(-n // chunk) for n in lens[multi]) and plan.n_items == plan.n_slots + (~multi).sum()
        assert (lens[multi] % chunk == 1).any() and (lens[multi] <= 2 * chunk).any()  # a last chunk of one entry; two chunks
        for alpha, reg in MODES:
            A64, b64, Aabs, cabs = refs[alpha, reg]
            tt, rhs = als.get_hermitian_implicit(plan, cg, vg, Yg, G, LAM, alpha, reg)
            tt2, rhs2 = als.get_hermitian_implicit(plan, cg, vg, Yg, G, LAM, alpha, reg)
            pk, prhs = als.get_hermitian_implicit_partial(plan, cg, vg, Yg, LAM, alpha, reg)
            pk2, prhs2 = als.get_hermitian_implicit_partial(plan, cg, vg, Yg, LAM, alpha, reg)
            tf = als.implicit_finish(pk, G, LAM if reg == "plain" else 0.0)
            torch.cuda.synchronize()
            tag = (f, chunk, alpha, reg)
            assert torch.equal(tt, tt2) and torch.equal(rhs, rhs2) and torch.equal(pk, pk2) and torch.equal(prhs, prhs2), tag
            t, r, p, pr, tfin = (v.cpu().numpy() for v in (tt, rhs, pk, prhs, tf))
            ratio = max((np.abs(t - A64) / Aabs).max(), (np.abs(tfin - A64) / Aabs).max(),
                        (np.abs(r - b64) / np.maximum(cabs, 1e-300)).max()) / 1e-5
            worst = max(worst, ratio)
            assert (np.abs(t - A64) <= 1e-5 * Aabs).all(), (tag, np.abs(t - A64).max())
            assert (np.abs(r - b64) <= 1e-5 * cabs + 1e-30).all(), (tag, np.abs(r - b64).max())
            tT = t.transpose(0, 2, 1)
            assert np.array_equal(t[:, off], tT[:, off]), tag
            assert (np.abs(t - tT) <= 2e-5 * Aabs).all(), tag  # diagonal tiles: two roundings of one value
            # packed mode
            assert (np.abs(tfin - A64) <= 1e-5 * Aabs).all(), (tag, np.abs(tfin - A64).max())
            assert (p[lens == 0] == 0).all() and (pr[lens == 0] == 0).all(), tag
            assert np.array_equal(pr, r), tag
            if reg == "plain":
                assert np.array_equal(tfin[~multi][:, iu[0], iu[1]], t[~multi][:, iu[0], iu[1]]), tag
        plan.close()
    print(f"implicit seams systems f={f} FT={-(-f // 16)}: largest error / bound {worst:.3f}")


# ---- 2. Gram at every tile count

@pytest.mark.parametrize("f", F_EDGES)
def test_gram_at_every_tile_count(alslib, f):
    """implicit_gram_partial_kernel<FT>: no rows, one stage, a ragged stage, exactly one slab of 1024 rows, one row into the
    second slab and one into the third; bound and checks of test_implicit_gram."""
    from cumf_als_amd import als

    Yall = _table(2049, f, 100 + f)
    worst = 0.0
    for rows in (0, 1, 33, 1024, 1025, 2049):
        Y = Yall[:rows]
        g = als.implicit_gram(_dev(Y)).cpu().numpy()
        g2 = als.implicit_gram(_dev(Y)).cpu().numpy()
        Y64 = Y.astype(np.float64)
        err, bound = np.abs(g - Y64.T @ Y64), 1e-5 * (np.abs(Y64).T @ np.abs(Y64))
        assert g.shape == (f, f) and (err <= bound).all(), (f, rows, err.max())
        assert np.array_equal(g, g2) and np.array_equal(g, g.T), (f, rows)
        if rows == 0:
            assert (g == 0).all(), f
        else:
            worst = max(worst, (err / bound).max())
    print(f"implicit seams gram f={f} FT={-(-f // 16)}: largest error / bound {worst:.3f}")


# ---- 3. the short-row CG at every length and at the lane seams

F_SHORT = [8, 30, 62, 64, 66, 96, 126, 128]  # f = 64: the last full one-feature lane, 66: two live lanes in the second half


@functools.lru_cache(maxsize=1)
def _short_rows():
    """Every row length 0..33 once (33 takes the Gram route), then 12 entries all negative (b = 0), 12 stored zeros (w = 0:
    A = G + reg I) and 32 entries all positive."""
    rng = np.random.RandomState(41)
    lens = np.array(list(rng.permutation(34)) + [12, 12, 32])
    rowptr, colidx, val = _csr(list(lens), N_TABLE, rng)
    val = val.copy()
    val[rowptr[34]:rowptr[35]] = rng.choice(VALUES[VALUES < 0], 12)
    val[rowptr[35]:rowptr[36]] = 0.0
    val[rowptr[36]:rowptr[37]] = rng.choice(VALUES[VALUES > 0], 32)
    return lens, rowptr, colidx, val


@pytest.mark.parametrize("f", F_SHORT)
def test_short_cg_every_length(oracle, alslib, f):
    """implicit_short_cg_kernel<TWO> with N = 8 / 16 / 32 at every row length.  One step: the result does not depend on the exit
    test, so every row is held on its own.  Three steps: the distribution rule, under the condition (asserted here, in fp64)
    that no row's r.r after step 1 or 2 is within a factor of 4 of the exit threshold."""
    lens, rowptr, colidx, val = _short_rows()
    assert sorted(lens[:34]) == list(range(34)) and len(lens) == 37
    Y = _table(N_TABLE, f, 3)
    x0 = _x0(len(lens), f)
    for alpha, reg in MODES:
        A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
        assert not b64[34].any() and not b64[35].any() and b64[36].any()
        tag = f"short f={f} alpha={alpha} {reg}"
        x64, x32 = _oracles(oracle, A64, b64, x0, f, 1)
        x, name = _update(rowptr, colidx, val, Y, x0, alpha, reg, "cg", 1)
        assert "implicit_short_cg_kernel" in name, name
        _check_rows(x, x64, x32, lens, tag + " iters=1")
        _assert_exit_clear(A64, b64, x0, lens, tag)
        x64, x32 = _oracles(oracle, A64, b64, x0, f, 3)
        x, _ = _update(rowptr, colidx, val, Y, x0, alpha, reg, "cg", 3)
        _check_dist(x, x64, x32, lens, tag + " iters=3")


@pytest.mark.parametrize("f", [8, 66])
def test_short_cg_grid_stride_pass(oracle, alslib, f):
    """The kernel launches at most 8192 workgroups of four waves; above 32 768 short rows its loop (k += gridDim.x * 4) takes a
    second trip.  40 000 rows: 64 template rows, with their own warm starts, 625 times.  A wave's arithmetic depends on its
    row only, so every copy returns the bits of the first; the first 64 rows are held to the one-step bound."""
    rng = np.random.RandomState(43)
    tl = rng.permutation(np.repeat(np.arange(1, 33), 2))
    reps = 625
    rp_t, ci_t, val_t = _csr(list(tl), N_TABLE, rng)
    lens = np.tile(tl, reps)
    assert len(lens) == 40_000 and ((lens > 0) & (lens <= 32)).sum() > 4 * 8192
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx, val = np.tile(ci_t, reps), np.tile(val_t, reps)
    Y = _table(N_TABLE, f, 3)
    x0_t = _x0(len(tl), f)
    x0 = np.tile(x0_t, (reps, 1))
    for alpha, reg in MODES:
        x, name = _update(rowptr, colidx, val, Y, x0, alpha, reg, "cg", 1)
        assert "implicit_short_cg_kernel" in name, name
        x = x.reshape(reps, len(tl), f)
        diff = np.flatnonzero((x != x[0]).any((1, 2)))
        assert len(diff) == 0, (f, alpha, diff[:10])
        A64, b64 = ref.systems(rp_t, ci_t, val_t, Y, LAM, alpha, reg)
        x64, x32 = _oracles(oracle, A64, b64, x0_t, f, 1)
        _check_rows(x[0], x64, x32, tl, f"grid-stride f={f} alpha={alpha} {reg} iters=1")


# ---- 4. the two routes on a mixed plan over a sub-range

ROW_BEGIN, ROW_END = 7, 53


@functools.lru_cache(maxsize=1)
def _mixed_rows():
    """60 rows, by row index modulo 4: empty, short (1..32), 33..64 (chunked at chunk = 32, whole at 64), 65..200 (chunked)."""
    rng = np.random.RandomState(47)
    lens = np.zeros(60, np.int64)
    lens[1::4] = rng.randint(1, 33, 15)
    lens[2::4] = rng.randint(33, 65, 15)
    lens[3::4] = rng.randint(65, 201, 15)
    lens[[9, 13, 10, 14, 18, 11, 15, 19]] = [32, 1, 33, 64, 63, 65, 129, 97]  # the seams, inside the range
    lens[[6, 7, 51, 53, 54]] = [64, 65, 129, 32, 33]  # both sides of the range's ends
    return (lens,) + _csr(list(lens), N_TABLE, rng)


@pytest.mark.parametrize("chunk", [32, 64])
@pytest.mark.parametrize("f", [8, 34, 64, 66, 100, 128])
def test_routes_on_a_mixed_sub_range(oracle, alslib, f, chunk):
    """The LU route's batch indexed by row - row_begin and the CG route's compact batch (longest-first item list ->
    d_long_row, item_dst, mrow_dst; gather, batched CG, scatter) with the short-row kernel and the zeroing of empty rows, on a
    plan of rows [7, 53) of 60: rows outside keep the bits of x0."""
    lens, rowptr, colidx, val = _mixed_rows()
    a, b = ROW_BEGIN, ROW_END
    inside = lens[a:b]
    assert (inside == 0).any() and ((inside > 0) & (inside <= 32)).any() and (inside > chunk).sum() >= 4
    assert ((inside > 32) & (inside <= chunk)).any() == (chunk == 64)  # whole long rows in the second case only
    assert (inside[inside > chunk] % chunk == 1).any()
    Y = _table(N_TABLE, f, 3)
    x0 = _x0(len(lens), f)

    def run(alpha, reg, solver, iters):
        x, name = _update(rowptr, colidx, val, Y, x0, alpha, reg, solver, iters, chunk, a, b)
        x2, _ = _update(rowptr, colidx, val, Y, x0, alpha, reg, solver, iters, chunk, a, b)
        tag = f"mixed f={f} chunk={chunk} alpha={alpha} {reg} {solver} iters={iters}"
        assert np.array_equal(x, x2), tag
        assert np.array_equal(x[:a], x0[:a]) and np.array_equal(x[b:], x0[b:]), tag
        assert ("implicit_short_cg_kernel" in name) == (solver == "cg"), (tag, name)
        return x[a:b], tag

    for alpha, reg in MODES:
        A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
        A64, b64, xs = A64[a:b], b64[a:b], x0[a:b]
        x, tag = run(alpha, reg, "lu", 0)
        _check_lu(x, A64, b64, oracle, inside, f, tag)
        x, tag = run(alpha, reg, "cg", 1)
        _check_rows(x, *_oracles(oracle, A64, b64, xs, f, 1), inside, tag)
        _assert_exit_clear(A64, b64, xs, inside, tag)
        x, tag = run(alpha, reg, "cg", 3)
        _check_dist(x, *_oracles(oracle, A64, b64, xs, f, 3), inside, tag)


@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_degenerate_plans(oracle, alslib, solver):
    """Every row short, no row short, every row empty, and an empty range, at f = 64: against the reference wherever a system
    exists (LU bound; one CG step, per row)."""
    f = 64
    rng = np.random.RandomState(53)
    Y = _table(N_TABLE, f, 3)
    iters = 0 if solver == "lu" else 1
    short = _csr(list(rng.randint(1, 33, 17)) + [1, 8, 9, 32], N_TABLE, rng)
    long_ = _csr(list(rng.randint(33, 200, 17)) + [33, 64, 65, 129], N_TABLE, rng)  # whole up to 64 entries, chunked above
    none = np.zeros(22, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    x0 = _x0(21, f)
    for alpha, reg in MODES:
        for kind, (rowptr, colidx, val), chunk in (("short", short, 0), ("long", long_, 64)):
            lens = np.diff(rowptr)
            x, name = _update(rowptr, colidx, val, Y, x0, alpha, reg, solver, iters, chunk)
            tag = f"degenerate all {kind} {solver} alpha={alpha} {reg}"
            assert ("implicit_short_cg_kernel" in name) == (kind == "short" and solver == "cg"), (tag, name)
            A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
            if solver == "lu":
                _check_lu(x, A64, b64, oracle, lens, f, tag)
            else:
                _check_rows(x, *_oracles(oracle, A64, b64, x0, f, 1), lens, tag)
            # an empty range: x untouched
            x, _ = _update(rowptr, colidx, val, Y, x0, alpha, reg, solver, iters, chunk, 5, 5)
            assert np.array_equal(x, x0), tag
        # every row empty: x = 0, and only inside the plan's range
        x, _ = _update(*none, Y, x0, alpha, reg, solver, iters)
        assert (x == 0).all()
        x, _ = _update(*none, Y, x0, alpha, reg, solver, iters, 0, 3, 17)
        assert (x[3:17] == 0).all() and np.array_equal(x[:3], x0[:3]) and np.array_equal(x[17:], x0[17:])


# ---- 5. the objective

@pytest.mark.parametrize("f", [8, 66, 130, 512])
def test_loss_small_and_wide(alslib, f):
    """cumf_implicit_loss on 37 x 53 (m < 4 x kImpLossBlocks: most workgroups own no row; two empty rows, one empty column),
    through the narrow Gram (f = 8, 66) and the wide one (f = 130, 512).  Tolerance: the project's 1e-6, of the sum of the
    absolute values of the terms (sparse_loss(absolute=True)), since the - s^2 terms may cancel the rest."""
    from cumf_als_amd import als

    m, n = 37, 53
    rng = np.random.RandomState(59)
    mask = rng.random_sample((m, n)) < 0.3
    mask[[4, m - 1]] = False
    mask[:, 17] = False
    assert (mask.sum(1) == 0).sum() == 2 and (mask.sum(0) == 0).sum() == 1
    R = np.full((m, n), np.nan)
    R[mask] = rng.choice(VALUES, mask.sum())
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
    colidx = np.concatenate([np.nonzero(mask[u])[0] for u in range(m)]).astype(np.int32)
    val = R[mask].astype(np.float32)  # row-major order = CSR order
    X, Y = _table(m, f, 1), _table(n, f, 2)
    rg, cg, vg, Xg, Yg = _dev(rowptr), _dev(colidx), _dev(val), _dev(X), _dev(Y)
    for alpha, reg in MODES:
        got = float(als.implicit_loss(rg, cg, vg, Xg, Yg, LAM, alpha, reg).item())
        got2 = float(als.implicit_loss(rg, cg, vg, Xg, Yg, LAM, alpha, reg).item())
        sparse = ref.sparse_loss(rowptr, colidx, val, X, Y, LAM, alpha, reg)
        dense = ref.dense_loss(R, X, Y, LAM, alpha, reg)
        L_abs = ref.sparse_loss(rowptr, colidx, val, X, Y, LAM, alpha, reg, absolute=True)
        print(f"implicit seams loss f={f} alpha={alpha} {reg}: got {got!r} sparse {sparse!r} dense {dense!r} "
              f"L_abs {L_abs!r} error / bound {abs(got - sparse) / (1e-6 * L_abs):.2e}")
        assert got == got2
        assert abs(got - sparse) <= 1e-6 * L_abs, (f, alpha, reg, got, sparse, L_abs)
        assert abs(got - dense) <= 1e-6 * L_abs, (f, alpha, reg, got, dense, L_abs)
