"""The diagonal tile of the sixteen-pivot one-wave LU (lu_wave_blocked16) exchanges FOUR pivot columns at a time: the copies
that every lane group keeps of columns 4 G .. 4 G + 3 take the same fma on the same operands as the registers of the owning
lane group, so the factors must be what they were before the change BIT FOR BIT.

tests/golden/lu16_exchange_parent.npz holds, for every case below, the factors that the commit before the change computed on
an MI355X for the same seeded inputs (`python tests/test_lu16_exchange_gpu.py OUT.npz` writes such a file with the library in
use), the name of the kernel that computed them and their per-row deviation from the fp64 oracle.  Each case is one
Theta-style LU half-iteration: a gather table of 64 rows (small enough for the pre-split planes, the production form of the
Theta side), 296 whole rows of 80, 81, 96, 97, 127, 128, 160 and 300 ratings -- all above the dual form's 79 and below one
chunk, on both sides of the 32-rating stage seams, several workgroups -- at f = 100 (the compile-time instance) and at the
run-time instances f = 98 and f = 110 (NB = 7, a last block row with 2 and 14 real pivots), lambda = 0.048 and 1e-5.  A row
longer than the table takes its columns from repeated shuffles of the table's rows.

Bounds: equality of the bits; and the per-row deviation from the fp64 oracle may not exceed the one recorded for the parent
(the oracle is recomputed here, the recorded deviation is against the same oracle code)."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lu16_exchange_parent.npz")
TABLE_ROWS = 64
LENS = (80, 81, 96, 97, 127, 128, 160, 300)
ROWS_PER_LEN = 37
FS = (100, 98, 110)
LAMS = (0.048, 1e-5)


def _key(f, lam):
    return f"f{f}_lam{lam:g}"


@functools.lru_cache(maxsize=None)
def _problem(f):
    """(rowptr, colidx, val, table, lens) of one feature count, seeded; read-only."""
    lens = tuple(n for n in LENS for _ in range(ROWS_PER_LEN))
    rng = np.random.RandomState(100 + f)
    table = (0.2 * rng.random_sample((TABLE_ROWS, f))).astype(np.float32)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cols = []
    for n in lens:
        shuffles = [rng.permutation(TABLE_ROWS) for _ in range((n + TABLE_ROWS - 1) // TABLE_ROWS)]
        cols.append(np.concatenate(shuffles)[:n])
    colidx = np.concatenate(cols).astype(np.int32)
    val = rng.randint(1, 6, size=len(colidx)).astype(np.float32)
    for a in (rowptr, colidx, val, table):
        a.setflags(write=False)
    return rowptr, colidx, val, table, lens


@functools.lru_cache(maxsize=None)
def _oracle(f, lam):
    from oracle import pyoracle

    pyoracle.build()
    rowptr, colidx, val, table, lens = _problem(f)
    x64 = np.zeros((len(lens), f), np.float32)  # the oracle computes in fp64 and stores fp32
    pyoracle.half_iteration(rowptr, colidx, val, table, x64, f, lam, solver="lu", dtype=np.float64)
    x64.setflags(write=False)
    return x64


def _run(f, lam):
    """One LU half-iteration on the GPU: the factors and the name of the kernel that solved the rows."""
    from cumf_als_amd import als

    rowptr, colidx, val, table, lens = _problem(f)
    x = torch.zeros((len(lens), f), device="cuda")
    plan = als.Plan(rowptr, f)
    assert plan.n_multi_rows == 0  # whole rows only
    als.update_fused(plan, torch.tensor(colidx).cuda(), torch.tensor(val).cuda(), torch.tensor(table).cuda(), x, lam, "lu")
    torch.cuda.synchronize()
    plan.close()
    return x.cpu().numpy(), als.last_kernel_name()


def _row_dev(x, x64):
    return np.abs(x - x64).max(axis=1) / np.abs(x64).max(axis=1)


def _record(out):
    """Write the fixture with the library in use (run at the commit whose factors are to be kept)."""
    data = {}
    for f in FS:
        for lam in LAMS:
            x, kernel = _run(f, lam)
            dev = _row_dev(x, _oracle(f, lam))
            print(f"{_key(f, lam)}: {kernel}  finite {np.isfinite(x).all()}  max per-row deviation from the fp64 oracle {dev.max():.3e}")
            data[_key(f, lam) + "_x"] = x.view(np.uint32)
            data[_key(f, lam) + "_dev"] = dev
            data[_key(f, lam) + "_kernel"] = np.array(kernel)
    np.savez(out, **data)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("f", FS)
def test_factors_are_the_parents_bit_for_bit(alslib, f, lam):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    g = _golden()
    x, kernel = _run(f, lam)
    want, want_dev, want_kernel = g[_key(f, lam) + "_x"], g[_key(f, lam) + "_dev"], str(g[_key(f, lam) + "_kernel"])
    assert kernel == want_kernel and "als_wave_kernel<7, 1, " + (str(f) if f == 100 else "0") + "," in kernel, (kernel, want_kernel)
    dev = _row_dev(x, _oracle(f, lam))
    lens = np.array(_problem(f)[4])
    print(f"{_key(f, lam)}: {kernel}")
    for n in LENS:
        print(f"  n={n:3d}: rows that differ from the parent {int((x.view(np.uint32)[lens == n] != want[lens == n]).any(1).sum())}"
              f"  max per-row deviation from the fp64 oracle {dev[lens == n].max():.3e}  parent {want_dev[lens == n].max():.3e}")
    assert np.isfinite(x).all()
    assert np.array_equal(x.view(np.uint32), want)
    assert (dev <= want_dev).all(), float((dev - want_dev).max())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _record(sys.argv[1])
