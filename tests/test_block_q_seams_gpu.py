"""The block solvers on the MI355X at Q = ceil(f / 64) = 4..7, at last blocks cut at and beside the 16-wide half, and row by
row: every live row within C_ROW x its own error scale (tests/block_ref.py: the spread of a family of float32 references
about the fp64 recurrence) with no absolute floor, so a long row cannot hide behind the error of a short one.  And the row
lists of the segmented route at more than one workgroup."""
import functools

import numpy as np
import pytest
import torch

from tests import block_ref as br
from tests.test_block_explicit_gpu import _check as pooled_check
from tests.test_block_nonneg_gpu import C as POOLED_C_NONNEG

pytestmark = pytest.mark.gpu

# the 8- and 16-entry tails of the opening reduction on both sides of its switch at Q = 4 / 5, a row of the 2048 class and a
# segmented row; the row-length seams themselves are tests/test_block_explicit_gpu.py's
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 65, 961, 2049]
N_COLS = 4200
SWEEPS = 2  # holds sweep 1, and the wrap of have_prev onto the ragged last block
# f: Q, width of the last block.  208: 4, 16; 256: 4, full (the profiled shape); 258: 5, 2 (the first f on the 8-entry
# reduction); 304: 5, 16 (last block at odd k); 366: 6, 14; 402: 7, 18; 448: 7, full
FS = (208, 256, 258, 304, 366, 402, 448)
ROUTES = [(f, "auto") for f in FS] + [(208, "segmented"), (304, "segmented")]
CUTS = [0, LENS.index(2049), len(LENS)]  # two plans: the rows the fused kernels take under "auto", and the longer one
# the implicit block solver has one route
CASES = [(kind, f, route) for f, route in ROUTES for kind in br.KINDS if route == "auto" or not kind.startswith("implicit")]


@functools.lru_cache(maxsize=None)
def _model(kind, f):
    return br.Model(kind, f, LENS, N_COLS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _update(m, route="auto", cuts=None, chunk=0):
    """The model's half-iteration through one plan per cut; returns (x, stats), stats the non-negative solver's."""
    from cumf_als_amd import als

    Yg, x, colidx, val = _dev(m.Y), _dev(m.x0.copy()), _dev(m.colidx), _dev(m.val)
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    G = unobserved = None
    if m.implicit:
        G = als.implicit_gram(Yg)
    elif m.kind == "rank1":
        unobserved = (_dev(m.own), _dev(m.gat))
        G = als.weighted_gram(Yg, unobserved[1])
    elif m.kind == "scalar":
        G = als.implicit_gram(Yg)
    cuts = cuts or [0, len(m.lens)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(m.rowptr, m.f, lo, hi, chunk)
        # the fused launches come last; a plan without a row of at most 2048 entries has none
        fused = route == "auto" and min(m.lens[lo:hi]) <= 2048
        if m.implicit:
            als.update_implicit(plan, colidx, val, Yg, G, x, br.LAM, m.alpha, m.reg, "block", SWEEPS)
            want = "block_row_kernel"
        elif m.weighted:
            als.update_weighted_block(plan, colidx, val, _dev(m.wgt), Yg, G, x, br.LAM, m.w0, m.reg, SWEEPS, route, unobserved)
            want = (("block_fused_gram_kernel", "block_row_kernel") if G is not None else
                    ("block_fused_kernel", "block_row_free_kernel"))[0 if fused else 1]
        else:
            if m.nonneg:
                als.update_block_nonneg(plan, colidx, val, Yg, x, br.LAM, SWEEPS, route, stats)
            else:
                als.update_block(plan, colidx, val, Yg, x, br.LAM, SWEEPS, route)
            want = "block_fused_kernel" if fused else "block_row_free_kernel"
        torch.cuda.synchronize()
        assert want in als.last_kernel_name(), (want, als.last_kernel_name())
        plan.close()
    return x.cpu().numpy(), stats.cpu().numpy()


def _check_rows(tag, m, x, stats, route):
    """x finite, every live row within C_ROW x its error scale, no floor; rows without entries exactly 0 (br.row_ratios)."""
    # G x is a chain in block_fused_gram_kernel, the rows of at most 2048 entries of the weighted model under "auto"
    chain_rows = (np.asarray(m.lens) <= 2048) & (route == "auto") & m.weighted
    ratio, use = br.row_ratios(tag, x, m, SWEEPS, chain_rows)
    left_out = m.live & ~use
    if m.nonneg:
        x64 = m.oracle(SWEEPS)[0]
        # a solver that ignores the constraint cannot pass: every live reference row has an exact zero and a positive coordinate
        assert ((x64[m.live] == 0).any(1) & (x64[m.live] > 0).any(1)).all()
        assert x.min() >= 0 and stats[0] == 0, (x.min(), stats)
        assert left_out.sum() <= m.live.sum() // 10, (tag, left_out)
        if left_out.any():  # a passive set jumped in a reference: that row answers to the pooled bound
            pooled_check(tag, x, x64, br.row_error_scale(m, SWEEPS, "pipe")[2], m.live, POOLED_C_NONNEG)
    assert use.sum() >= m.live.sum() - m.live.sum() // 10, (tag, use)
    assert (ratio[use] <= br.C_ROW).all(), (tag, np.round(ratio, 3).tolist())


@pytest.mark.parametrize("kind,f,route", CASES)
def test_block_rows_at_q_seams(alslib, kind, f, route):
    m = _model(kind, f)  # the references of one (f, model) are computed once: block_ref caches them per model
    x, stats = _update(m, route, CUTS)
    _check_rows(f"{kind} f={f} {route}", m, x, stats, route)


def test_block_bits_at_q5(alslib):
    """f = 304 (Q = 5, a 16-wide last block at odd k): the fused and the segmented route where they share their sums, three
    plans and the plan's chunks, bit-identical factors and statistics."""
    f, rows = 304, len(LENS)
    for kind in br.KINDS:
        m = _model(kind, f)
        want, stats = _update(m)
        variants = [{"cuts": [0, rows // 3, 2 * rows // 3, rows]}, {"chunk": 1000}]
        if kind in ("explicit", "nonneg", "w0=0"):  # no Gram term: a row's bits do not depend on the route
            variants += [{"route": "segmented"}, {"cuts": [0, 7, rows], "chunk": 1000, "route": "segmented"}]
        for kw in variants:
            x, st = _update(m, **kw)
            assert np.array_equal(x, want) and np.array_equal(st, stats), (kind, kw)
        if m.nonneg:
            assert stats[0] == 0 and stats[1] > 0, stats


# ---- the row lists of the segmented route: block_row_kernel takes 32 rows of the list per workgroup, block_row_free_kernel four
LIST_LENS = [[0, 1, 5, 33, 64, 70][r % 6] for r in range(70)]
LIST_F = 66


@functools.lru_cache(maxsize=None)
def _list_model(kind):
    return br.Model(kind, LIST_F, LIST_LENS, N_COLS)


@pytest.mark.parametrize("kind", ["scalar", "rank1", "explicit"])
def test_row_list_second_workgroup(alslib, kind):
    """70 rows, 12 of them without entries.  Under "segmented" the plan lists every row of its range as a long row, the empty
    ones too (the list kernels write their zeros), so the list holds 70 rows: workgroups of 32, 32 and 6 rows in
    block_row_kernel (scalar, rank1), seventeen of four rows and one of two in block_row_free_kernel (explicit).  Plans cut
    at 7 and 39 start inside the one plan's first workgroup and end inside its second: the same bits, and every row within
    its bound."""
    m = _list_model(kind)
    x, stats = _update(m, "segmented")
    cut, _ = _update(m, "segmented", cuts=[0, 7, 39, 70])
    assert np.array_equal(cut, x)
    _check_rows(f"row list {kind} f={LIST_F} segmented", m, x, stats, "segmented")
