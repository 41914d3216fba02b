"""The references of tests/block_ref.py against each other, on the CPU: block_sparse32 (the kernels' form in float32) against
the fp64 dense recurrence for every model, a held-out entry order against the per-row bound the kernels are held to, and the
non-negative model's rows left out of that bound, for the reference family alone."""
import functools

import numpy as np
import pytest

from tests import block_ref as br

LENS = [0, 1, 7, 8, 9, 15, 16, 17, 65, 961, 2049]  # tests/test_block_q_seams_gpu.py's rows
N_COLS = 4200
SEAM_F = (208, 256, 258, 304, 366, 402, 448)
SWEEPS = 2


@functools.lru_cache(maxsize=None)
def _model(kind, f):
    return br.Model(kind, f, LENS, N_COLS)


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("f", [34, 66])
def test_sparse_form_is_the_recurrence(kind, f):
    """block_sparse32 is the dense recurrence in another order of summation: run in fp64 it agrees with the fp64 oracle to
    fp64 rounding (1e-11 of the factors' scale: 2^-53 x some 1e3 terms x a condition number below 1e2), in both forms of the
    Gram term and with the same passive sets; in float32 it is a float32 result (the ratio to the dense float32 members is
    printed)."""
    m = _model(kind, f)
    x64, sets64 = m.oracle(SWEEPS)
    scale = np.abs(x64).max()
    E = np.max([br.row_distance(x, x64) for _, x, _ in m.dense_members(SWEEPS)], axis=0)
    for gram in ("chain", "pipe") if m.has_gram else ("chain",):
        x, sets = m.sparse32(SWEEPS, gram, np.float64)
        assert (x[~m.live] == 0).all()
        assert np.abs(x - x64).max() <= 1e-11 * scale, (kind, f, gram, np.abs(x - x64).max())
        assert not m.jumped(sets, SWEEPS).any()
        x = m.sparse32(SWEEPS, gram)[0]
        assert x.dtype == np.float32 and (x[~m.live] == 0).all()
        with np.errstate(divide="ignore"):  # a row whose weights are all 0 has the dense members exact
            print(f"sparse32/{gram} {kind} f={f}: per-row ratio to the dense float32 members "
                  f"{np.round(br.row_distance(x, x64)[m.live] / E[m.live], 2).tolist()}")
        assert np.abs(x - x64).max() <= 1e-5 * scale


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("f", [34, 66, 208])
def test_held_out_order_meets_the_row_bound(kind, f):
    """An entry order the family does not hold: the reference alone meets the bound the kernels are held to."""
    m = _model(kind, f)
    x, sets = m.dense(np.float32, SWEEPS, br.N_ORDERS + 1)
    E, left_out, _ = br.row_error_scale(m, SWEEPS, "pipe")
    use = m.live & ~left_out & ~m.jumped(sets, SWEEPS)
    err = br.row_distance(x, m.oracle(SWEEPS)[0])[use]
    ratio = np.divide(err, E[use], out=np.zeros_like(err), where=err > 0)
    print(f"held-out order {kind} f={f}: per-row ratio {np.round(ratio, 3).tolist()}")
    assert use.sum() >= m.live.sum() - m.live.sum() // 10
    assert (ratio <= br.C_ROW).all(), (kind, f, ratio.max())


@pytest.mark.parametrize("kind", [k for k in br.KINDS if k.startswith("implicit") or k in ("scalar", "rank1")])
@pytest.mark.parametrize("f", [34, 66, 208])
def test_held_out_gram_order_meets_the_row_bound(kind, f):
    """A summation order of G the family does not hold (gram_slabs on a further order of the table's rows), in both forms of
    G x: the family with its slab-summed members meets its own bound without any kernel."""
    m = _model(kind, f)
    x64 = m.oracle(SWEEPS)[0]
    for gram in ("chain", "pipe"):
        x = m.sparse32(SWEEPS, gram, slabs=br.N_GRAMS_SHORT)[0]
        E = br.row_error_scale(m, SWEEPS, gram)[0]
        err = br.row_distance(x, x64)[m.live]
        with np.errstate(divide="ignore"):
            ratio = np.divide(err, E[m.live], out=np.zeros_like(err), where=err > 0)
        print(f"held-out G order {kind} f={f} {gram}: per-row ratio {np.round(ratio, 3).tolist()}")
        assert np.isfinite(x).all() and (x[~m.live] == 0).all()
        assert (ratio <= br.C_ROW).all(), (kind, f, gram, ratio.max())


@pytest.mark.parametrize("f", SEAM_F)
def test_nonneg_rows_left_out(f):
    """The non-negative model at the GPU test's shapes: every live fp64 row has an exact zero and a positive coordinate, and
    the family leaves at most one live row in ten out of the per-row bound."""
    m = _model("nonneg", f)
    x64 = m.oracle(SWEEPS)[0]
    assert ((x64[m.live] == 0).any(1) & (x64[m.live] > 0).any(1)).all()
    E, left_out, _ = br.row_error_scale(m, SWEEPS)
    print(f"nonneg f={f}: rows left out {np.flatnonzero(left_out).tolist()} of {int(m.live.sum())} live")
    assert left_out.sum() <= m.live.sum() // 10
    assert (E[m.live & ~left_out] > 0).all()
