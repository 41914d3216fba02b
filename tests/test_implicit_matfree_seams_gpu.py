"""The matrix-free implicit CG (solver "cg_matfree") and the wide Gram at the seams tests/test_implicit_matfree_gpu.py leaves out:
every lane-group count Q = ceil(f / 64) with a partly filled last lane group and a ragged 16-column tile count, a partial row
workgroup, rows at the 2048-entry segment cut, the early exit, more segments than the sparse pass has waves, the plan's
chunk, and Gram tables longer than one slab.  Reference and bound are those of test_update_implicit_matfree throughout."""
import functools

import numpy as np
import pytest
import torch

from tests import implicit_ref as ref
from tests.test_implicit_matfree_gpu import _dev, _stats, _table

pytestmark = pytest.mark.gpu

LAM = 0.05
VALUES = np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0], np.float32)  # the ratings of _mixed(): negatives, stored zeros
N_COLS = 5000  # gather table rows: enough to draw 4097 distinct columns
F_SEAMS = [10, 62, 66, 190, 258, 318, 322, 386, 446, 450, 510]  # Q = 1, 1, 2, 3, 5, 5, 6, 7, 7, 8, 8
# first row workgroup (kFreeRows = 32 rows): an empty row, the N = 8 / N = 16 block tails and the segment cut at kFreeSeg = 2048
LENS_A = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 72, 2047, 2048, 4096]
# second one, 13 rows (nr < kFreeRows): an empty row and the rows one past a full segment
LENS_B = [0, 2049, 4097]
CG_EXIT = 1e-4  # the r.r below which a row's CG ends (CG_ERROR of the reference's cg.cu)


def _csr(lens, n_cols, rng):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(n_cols, ln, replace=False)) for ln in lens]).astype(np.int32)
    val = rng.choice(VALUES, int(rowptr[-1]))
    return rowptr, colidx, val


@functools.lru_cache(maxsize=1)
def _seam_rows():
    """45 rows: 32 in the first row workgroup, 13 in the second."""
    rng = np.random.RandomState(17)
    lens = LENS_A + list(rng.randint(1, 120, 32 - len(LENS_A))) + LENS_B + list(rng.randint(1, 120, 13 - len(LENS_B)))
    assert len(lens) == 45 and lens[:32].count(0) == 1 and lens[32:].count(0) == 1
    return (np.asarray(lens),) + _csr(lens, N_COLS, rng)


class _Side:
    """The device copies one case's updates share: entries, gather table and its Gram."""

    def __init__(self, rowptr, colidx, val, Y):
        from cumf_als_amd import als

        self.rowptr, self.f = rowptr, Y.shape[1]
        self.colidx, self.val, self.Y = _dev(colidx), _dev(val), _dev(Y)
        self.G = als.implicit_gram(self.Y)

    def update(self, x0, alpha, reg, iters, cuts=None, chunk=0):
        """x0 updated by "cg_matfree" through one plan per row range of `cuts`; returns x and the last kernel's name."""
        from cumf_als_amd import als

        rows = len(self.rowptr) - 1
        cuts = [0, rows] if cuts is None else cuts
        x = _dev(x0.copy())
        for a, b in zip(cuts[:-1], cuts[1:]):
            plan = als.Plan(self.rowptr, self.f, row_begin=a, row_end=b, chunk=chunk)
            als.update_implicit(plan, self.colidx, self.val, self.Y, self.G, x, LAM, alpha, reg, "cg_matfree", iters)
            torch.cuda.synchronize()
            name = als.last_kernel_name()
            plan.close()
        return x.cpu().numpy(), name


def _check(x, x64, x32, lens, f, tag):
    """The bound of test_update_implicit_matfree: median / q90 / max of the per-row max-norm distance to the fp64 oracle.cg
    within c x those of the fp32 oracle.cg + 1e-5 of the scale, c = 1.05 at f <= 128 and 2 above; empty rows exactly 0.  And
    every row of at least 2047 entries on its own within c x the fp32 oracle's largest row error + 1e-5 of the scale, so
    that one wrong long row cannot hide in the statistics.  Returns the largest of the three ratios."""
    c = 1.05 if f <= 128 else 2.0
    empty = lens == 0
    assert (x[empty] == 0).all(), tag
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1), np.abs(x32 - x64).max(1)
    s_h, s_o = _stats(e_h[~empty]), _stats(e_o[~empty])
    ratio = max(h / o for h, o in zip(s_h, s_o) if o > 0)
    print(f"implicit cg_matfree {tag}: hip {s_h} oracle32 {s_o} ratio {ratio:.3f}")
    for h, o in zip(s_h, s_o):
        assert h <= c * o + 1e-5 * scale, (tag, s_h, s_o)
    for u in np.flatnonzero(lens >= 2047):
        assert e_h[u] <= c * s_o[2] + 1e-5 * scale, (tag, int(u), int(lens[u]), float(e_h[u]), s_o)
    return ratio


def _oracles(oracle, A64, b64, x0, f, iters):
    x64 = oracle.cg(A64, x0.astype(np.float64), b64, f, iters)
    x32 = oracle.cg(A64.astype(np.float32), x0, b64.astype(np.float32), f, iters)
    return x64, x32


@pytest.mark.parametrize("f", F_SEAMS)
def test_matfree_every_lane_group_count(oracle, alslib, f):
    """Every Q = 1..8 of implicit_free_sparse_kernel<Q> / implicit_free_row_kernel<Q>; Q = 5, 6, 7 (N = 8 entries per block)
    with f % 64 != 0 and f % 16 != 0, f = 258 with two live lanes in the last lane group and FT = 17 tiles over four waves,
    f = 510 at Q = 8 with f % 16 = 14."""
    lens, rowptr, colidx, val = _seam_rows()
    Y = _table(N_COLS, f, 3)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
    side = _Side(rowptr, colidx, val, Y)
    worst = 0.0
    for alpha in (1.0, 40.0):
        for reg in ("weighted", "plain"):
            A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
            for iters in (1, 6):
                x64, x32 = _oracles(oracle, A64, b64, x0, f, iters)
                x, name = side.update(x0, alpha, reg, iters)
                assert "implicit_free_row_kernel" in name, name
                worst = max(worst, _check(x, x64, x32, lens, f, f"f={f} iters={iters} alpha={alpha} {reg}"))
    print(f"implicit cg_matfree seams f={f}: largest ratio to the fp32 oracle {worst:.3f} (bound {1.05 if f <= 128 else 2.0})")


# ---- early exit

def _cg_rs(A, x0, b, iters):
    """The CG recurrence of cumf_cg_solve_batched / implicit_free_row_kernel in plain fp64: r.r after the start and after
    every step taken, and the step at which the row ends (r.r < CG_EXIT is tested after each step, never at the start)."""
    x = x0.astype(np.float64)
    r = b - A @ x
    p = r.copy()
    rs = [float(r @ r)]
    for k in range(1, iters + 1):
        ap = A @ p
        a = rs[-1] / (p @ ap)
        x += a * p
        r -= a * ap
        rs.append(float(r @ r))
        if rs[-1] < CG_EXIT:
            return rs, k
        p = r + (rs[-1] / rs[-2]) * p
    return rs, iters


def _exit_case(f):
    """41 rows.  Workgroup 0 (rows 0..31) interleaves three kinds by row index: "fast" rows whose warm start is the solution
    plus an error along ONE eigenvector of A_u (CG ends it in one step), "mid" rows with an error along two or three
    eigenvectors (alternately; the smallest, the largest and the middle eigenvalue, so two or three steps and not one fewer),
    "slow" rows with a large random warm start.  Workgroup 1 (rows 32..40) holds only fast rows and an empty one, so all its
    rows are done after step 1.  One fast and one slow row are two segments long.  alpha = 1 keeps b, and with it the fp32
    rounding floor of r.r, far below CG_EXIT.  The table's columns are scaled over a decade so that G alone is
    ill-conditioned enough to keep the slow rows going."""
    rng = np.random.RandomState(11)
    n_cols, alpha = 2500, 1.0
    kinds = [("fast", "mid", "slow")[u % 3] for u in range(32)] + ["fast"] * 9
    lens = list(rng.randint(20, 90, len(kinds)))
    lens[0] = lens[2] = 2100
    lens[36] = 0
    rowptr, colidx, val = _csr(lens, n_cols, rng)
    Y = (0.3 * rng.standard_normal((n_cols, f)) * np.logspace(0, -1, f)).astype(np.float32)
    A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, "weighted")
    x0 = np.zeros((len(lens), f), np.float32)
    steps = np.zeros(len(lens), np.int64)  # the step each row is built to end at (6: never within 6)
    n_mid = 0
    for u, kind in enumerate(kinds):
        if lens[u] == 0 or kind == "slow":
            x0[u] = 0.5 * rng.standard_normal(f)
            steps[u] = 0 if lens[u] == 0 else 6
            continue
        lam, U = np.linalg.eigh(A64[u])
        if kind == "fast":
            pick = [rng.randint(f)]
        else:
            pick = [[0, f - 1], [0, f // 2, f - 1]][n_mid % 2]
            n_mid += 1
        steps[u] = len(pick)
        # a residual of 3 along each picked eigenvector
        x0[u] = np.linalg.solve(A64[u], b64[u]) + 3.0 * sum(U[:, i] / lam[i] for i in pick)
    return np.asarray(lens), kinds, rowptr, colidx, val, Y, alpha, A64, b64, x0, steps


@pytest.mark.parametrize("f", [258, 64])
def test_matfree_early_exit_freezes_rows(oracle, alslib, f):
    lens, kinds, rowptr, colidx, val, Y, alpha, A64, b64, x0, steps = _exit_case(f)
    # the inputs do what they are built for, in fp64: every row ends at its step, and no r.r that is compared with CG_EXIT lies
    # within a factor of 4 of it, so the fp32 kernel ends each row at the same step
    for u in np.flatnonzero(lens > 0):
        rs, k = _cg_rs(A64[u], x0[u], b64[u], 6)
        assert k == steps[u], (u, kinds[u], k, rs)
        assert all(v < CG_EXIT / 4 or v > CG_EXIT * 4 for v in rs[1:]), (u, kinds[u], rs)
        assert (rs[-1] < CG_EXIT / 4) == (kinds[u] != "slow"), (u, kinds[u], rs)
    assert {kinds[u] for u in range(32)} == {"fast", "mid", "slow"} and set(steps[32:]) <= {0, 1}
    assert set(steps[[u for u in range(32) if kinds[u] == "mid"]]) == {2, 3}

    side = _Side(rowptr, colidx, val, Y)
    got = {it: side.update(x0, alpha, "weighted", it)[0] for it in (1, 2, 3, 6)}
    x64, x32 = _oracles(oracle, A64, b64, x0, f, 6)
    _check(got[6], x64, x32, lens, f, f"early exit f={f} iters=6")
    for s in (1, 2, 3):
        rows = np.flatnonzero(steps == s)
        assert len(rows) > 0
        # a row that ended at step s is never touched again
        assert np.array_equal(got[6][rows], got[s][rows]), (s, rows[(got[6][rows] != got[s][rows]).any(1)])
    slow = np.flatnonzero(steps == 6)
    assert (got[6][slow] != got[3][slow]).any(1).all()  # ... while the others went on


# ---- more segments than the sparse pass has waves

def test_matfree_second_grid_trip(oracle, alslib):
    """The sparse pass launches at most 16384 workgroups of four waves: above 65536 segments its grid-stride loop takes a
    second trip.  70 000 one-segment rows in one plan, against the same rows through two plans that stay under the cap."""
    f, alpha, reg, rows = 8, 40.0, "weighted", 70_000
    rng = np.random.RandomState(23)
    lens = rng.randint(1, 4, rows)
    lens[[0, 31, 34_999, 35_000, 65_536, rows - 1]] = 0
    assert (lens > 0).sum() > 4 * 16384 and (lens[:35_000] > 0).sum() < 4 * 16384 and (lens[35_000:] > 0).sum() < 4 * 16384
    n_cols = 2000
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = (rng.randint(0, n_cols - 14, rows)[:, None] + 7 * np.arange(3))[np.arange(3) < lens[:, None]].astype(np.int32)
    val = rng.choice(VALUES, int(rowptr[-1]))
    Y = _table(n_cols, f, 3)
    x0 = (0.05 * rng.standard_normal((rows, f))).astype(np.float32)
    A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
    x64, x32 = _oracles(oracle, A64, b64, x0, f, 3)
    side = _Side(rowptr, colidx, val, Y)
    x, _ = side.update(x0, alpha, reg, 3)
    _check(x, x64, x32, lens, f, f"{rows} rows f={f} iters=3")
    x2, _ = side.update(x0, alpha, reg, 3, cuts=[0, 35_000, rows])
    assert np.array_equal(x, x2), np.flatnonzero((x != x2).any(1))[:10]


# ---- the plan's chunk

@pytest.mark.parametrize("f", [258, 190])
def test_matfree_ignores_the_plan_chunk(alslib, f):
    """The segments are cut every kFreeSeg entries from the row's start, whatever chunks the plan cut the row into.  f = 190
    besides f = 258: up to f = 207 the plan really cuts its rows at `chunk` (above, an item is always a whole row), so only
    there do the long rows reach the segment list as many items in longest-first order."""
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _seam_rows()
    Y = _table(N_COLS, f, 3)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
    side = _Side(rowptr, colidx, val, Y)
    want, _ = side.update(x0, 40.0, "weighted", 6)
    for chunk in (64, 2048):
        got, _ = side.update(x0, 40.0, "weighted", 6, chunk=chunk)
        assert np.array_equal(got, want), (f, chunk, np.flatnonzero((got != want).any(1)))
    if f == 190:
        cut, whole = als.Plan(rowptr, f, chunk=64), als.Plan(rowptr, f, chunk=8192)
        assert cut.n_items > whole.n_items == len(lens), (cut.n_items, whole.n_items)
        cut.close()
        whole.close()


# ---- the wide Gram across slabs

@pytest.mark.parametrize("f", [258, 322, 386, 450, 510, 512])
def test_implicit_gram_wide_across_slabs(alslib, f):
    """One workgroup column of the wide Gram takes `slab` table rows and writes one FP x FP partial; the partials are summed in
    slab order.  slab = 1024 ceil(FT / 8), FT = ceil(f / 16), is implicit_gram_slab() of csrc/als_implicit.h above f = 128."""
    from cumf_als_amd import als

    FT = -(-f // 16)
    slab = 1024 * -(-FT // 8)
    assert slab == (3072 if f <= 384 else 4096)
    Yall = _table(2 * slab + 33, f, f)
    got = {}
    for rows in (33, slab - 1, slab, slab + 1, 2 * slab + 33):  # prefixes of one table
        Y = Yall[:rows]
        g = als.implicit_gram(_dev(Y)).cpu().numpy()
        g2 = als.implicit_gram(_dev(Y)).cpu().numpy()
        Y64 = Y.astype(np.float64)
        bound = 1e-5 * (np.abs(Y64).T @ np.abs(Y64))
        err = np.abs(g - Y64.T @ Y64)
        assert (err <= bound).all(), (f, rows, err.max())
        assert np.array_equal(g, g2) and np.array_equal(g, g.T), (f, rows)
        got[rows] = g, bound
    # the row that starts the second slab is not dropped
    y = Yall[slab].astype(np.float64)
    err = np.abs(got[slab + 1][0] - (got[slab][0].astype(np.float64) + np.outer(y, y)))
    assert (err <= got[slab + 1][1]).all(), (f, err.max())


# ---- limits

def test_matfree_limits(alslib):
    from cumf_als_amd import als

    for f in (6, 7, 129, 511, 513, 514):
        assert not als.implicit_available(f, "cg_matfree"), f
    for f in (8, 130, 510, 512):
        assert als.implicit_available(f, "cg_matfree"), f
    rng = np.random.RandomState(5)
    lens = [3, 0, 40, 5]
    rowptr, colidx, val = _csr(lens, 64, rng)
    for f in (6, 7, 129, 511, 513, 514):
        try:
            plan = als.Plan(rowptr, f)
        except RuntimeError:
            # no plan exists for an odd f or one above 512: a plan of another f, handed over as one of f, must be refused too
            plan = als.Plan(rowptr, 8)
            plan.f = f
        x0 = _table(len(lens), f, f)
        x = _dev(x0.copy())
        G = torch.zeros((f, f), dtype=torch.float32, device="cuda")
        with pytest.raises(RuntimeError, match="cumf_als_update_implicit"):
            als.update_implicit(plan, _dev(colidx), _dev(val), _dev(_table(64, f, 1)), G, x, LAM, 40.0, "weighted",
                                "cg_matfree", 3)
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), x0), f
        plan.close()
