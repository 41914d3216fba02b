"""Short whole rows of an LU half-iteration in their n x n dual form (als_dual.hip) against the fp64 oracle and against the
primal route (CUMF_ALS_DUAL=0) of the same process.

Tolerances: the project's LU tolerance, 1e-4 of the row's scale per row (tests/test_gpu_parity.py), and no more than twice
the primal route's own distance from the fp64 oracle on the same rows; rows the route must not take are bit-identical to
the primal route.  Fused train SSE: 2e-5 relative against the RMSE kernel (test_fused_train_sse_matches_the_rmse_kernel)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TABLE_ROWS = 300
LAM = 0.05
LENS = [1, 2, 15, 16, 17, 33, 47, 48, 49, 63, 64, 65, 78, 79, 80, 81]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


def _table(f, seed=1):
    rng = np.random.RandomState(seed)
    return (0.2 * rng.random_sample((TABLE_ROWS, f))).astype(np.float32)


def _csr(lens, seed=2):
    """Rows of the given lengths: distinct table rows per row, ratings 1 .. 5."""
    rng = np.random.RandomState(seed)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([rng.choice(TABLE_ROWS, n, replace=False) for n in lens] + [[]]).astype(np.int32)
    val = rng.randint(1, 6, size=len(colidx)).astype(np.float32)
    return rowptr, colidx, val


@functools.lru_cache(maxsize=None)
def _problem(f, lens):
    """(rowptr, colidx, val, table, x64): the fp64 oracle half-iteration, computed once per shape."""
    from oracle import pyoracle

    pyoracle.build()
    rowptr, colidx, val = _csr(list(lens))
    table = _table(f)
    x64 = np.zeros((len(lens), f), np.float32)  # the oracle computes in fp64 and stores fp32
    pyoracle.half_iteration(rowptr, colidx, val, table, x64, f, LAM, solver="lu", dtype=np.float64)
    for a in (rowptr, colidx, val, table, x64):
        a.setflags(write=False)
    return rowptr, colidx, val, table, x64


def _run(f, rowptr, colidx, val, table, sse=False, batches=1):
    """One LU half-iteration on the GPU: the factors (and the SSE bins' sum)."""
    from cumf_als_amd import als

    rows = len(rowptr) - 1
    x = torch.zeros((rows, f), device="cuda")
    ci, va, tb = torch.tensor(colidx).cuda(), torch.tensor(val).cuda(), torch.tensor(table).cuda()
    total = 0.0
    for b in range(batches):
        plan = als.Plan(rowptr, f, rows * b // batches, rows * (b + 1) // batches)
        if sse:
            assert als.fused_sse_available(plan, "lu")
            total += float(als.update_fused_sse(plan, ci, va, tb, x, LAM, "lu").sum().item())
        else:
            als.update_fused(plan, ci, va, tb, x, LAM, "lu")
        torch.cuda.synchronize()
        plan.close()
    return (x.cpu().numpy(), total) if sse else x.cpu().numpy()


def _both_routes(monkeypatch, f, rowptr, colidx, val, table, **kw):
    monkeypatch.delenv("CUMF_ALS_DUAL", raising=False)
    dual = _run(f, rowptr, colidx, val, table, **kw)
    monkeypatch.setenv("CUMF_ALS_DUAL", "0")
    primal = _run(f, rowptr, colidx, val, table, **kw)
    monkeypatch.delenv("CUMF_ALS_DUAL")
    return dual, primal


def _row_dev(x, x64):
    return np.abs(x - x64).max(axis=1) / np.abs(x64).max(axis=1)


def _routed(f, rowptr):
    from cumf_als_amd import als

    plan = als.Plan(rowptr, f)
    chunk = plan.chunk
    plan.close()
    return als.dual_rows_probe(rowptr, f, chunk, "lu", gather_rows=TABLE_ROWS)["routed"]


@pytest.mark.parametrize("f,lens", [(100, tuple(LENS)), (96, (16, 64, 79)), (108, (16, 64, 79))])
def test_dual_rows_against_the_fp64_oracle_and_the_primal_route(alslib, monkeypatch, f, lens):
    _need_gpu()
    lens3 = tuple(n for n in lens for _ in range(3))
    rowptr, colidx, val, table, x64 = _problem(f, lens3)
    taken = np.array([n <= 79 for n in lens3])
    # f = 108 has no pre-split table (a strip of twelve features): the route declines and every row stays primal
    assert _routed(f, rowptr) == (0 if f == 108 else int(taken.sum()))
    xd, xp = _both_routes(monkeypatch, f, rowptr, colidx, val, table)
    assert np.isfinite(xd).all() and np.isfinite(xp).all()
    dd, dp = _row_dev(xd, x64), _row_dev(xp, x64)
    print(f"dual rows f={f}: max per-row relative deviation from the fp64 oracle on the rows of <= 79 ratings: "
          f"dual {dd[taken].max():.3e}  primal {dp[taken].max():.3e}  (all rows: {dd.max():.3e} / {dp.max():.3e})")
    for n in sorted(set(lens3)):
        sel = np.array(lens3) == n
        print(f"  n={n:3d}: dual {dd[sel].max():.3e}  primal {dp[sel].max():.3e}")
    assert dd.max() <= 1e-4, dd.max()
    assert dd[taken].max() <= 2.0 * dp[taken].max(), (dd[taken].max(), dp[taken].max())
    # rows of 80 ratings or more must not be taken: the bits of the primal route
    assert np.array_equal(xd[~taken].view(np.uint32), xp[~taken].view(np.uint32))
    if f != 108:  # ... and the dual kernel did run on the others (another system is factored: other bits somewhere)
        assert not np.array_equal(xd[taken].view(np.uint32), xp[taken].view(np.uint32))


def test_degenerate_rows(alslib, monkeypatch):
    """All gathered rows equal; only zero rows gathered (x = 0 exactly); a ratings-free row next to short rows (NaN as the
    reference's unpivoted LU gives, the other rows untouched by it)."""
    _need_gpu()
    from oracle import pyoracle

    f = 100
    lens = [40, 33, 0, 20, 79]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rng = np.random.RandomState(3)
    colidx = np.concatenate([np.full(40, 7), np.arange(33), rng.choice(np.arange(50, TABLE_ROWS), 20, replace=False),
                             rng.choice(np.arange(50, TABLE_ROWS), 79, replace=False)]).astype(np.int32)
    val = rng.randint(1, 6, size=len(colidx)).astype(np.float32)
    table = _table(f).copy()
    table[:33] = 0.0
    table[7] = 0.1 + 0.01 * np.arange(f, dtype=np.float32)
    colidx[40:73] = np.r_[0:7, 8:34]  # row 1 gathers zero rows only (row 7 of the table is the one row 0 repeats)
    table[33] = 0.0
    assert _routed(f, rowptr) == 4
    xd, xp = _both_routes(monkeypatch, f, rowptr, colidx, val, table)
    assert np.array_equal(np.isnan(xd), np.isnan(xp)) and np.isnan(xd[2]).all() and np.isfinite(xd[[0, 1, 3, 4]]).all()
    assert (xd[1] == 0.0).all()
    x64 = np.zeros((len(lens), f), np.float32)  # the oracle computes in fp64 and stores fp32
    pyoracle.half_iteration(rowptr, colidx, val, table, x64, f, LAM, solver="lu", dtype=np.float64)
    ok = [0, 3, 4]
    dd, dp = _row_dev(xd[ok], x64[ok]), _row_dev(xp[ok], x64[ok])
    print(f"degenerate rows: per-row relative deviation dual {dd}  primal {dp}")
    assert dd.max() <= 1e-4 and dd.max() <= 2.0 * dp.max(), (dd, dp)


def test_fused_train_sse_of_dual_rows(alslib, monkeypatch):
    _need_gpu()
    from cumf_als_amd import als

    f = 100
    lens3 = tuple(n for n in LENS for _ in range(3))
    rowptr, colidx, val, table, _ = _problem(f, lens3)
    monkeypatch.delenv("CUMF_ALS_DUAL", raising=False)
    x, fused = _run(f, rowptr, colidx, val, table, sse=True)
    row = np.repeat(np.arange(len(lens3)), np.diff(rowptr)).astype(np.int32)
    kern = float(als.sse(torch.tensor(val).cuda(), torch.tensor(row).cuda(), torch.tensor(colidx).cuda(),
                         torch.tensor(table).cuda(), torch.tensor(x).cuda()).item())
    print(f"fused train SSE with dual rows: fused {fused:.6f}  kernel {kern:.6f}  rel {abs(fused - kern) / kern:.2e}")
    assert abs(fused - kern) <= 2e-5 * kern, (fused, kern)


def test_batched_plans_are_bit_identical(alslib, monkeypatch):
    _need_gpu()
    f = 100
    lens3 = tuple(n for n in LENS for _ in range(3))
    rowptr, colidx, val, table, _ = _problem(f, lens3)
    monkeypatch.delenv("CUMF_ALS_DUAL", raising=False)
    x1 = _run(f, rowptr, colidx, val, table)
    x3 = _run(f, rowptr, colidx, val, table, batches=3)
    assert np.array_equal(x1.view(np.uint32), x3.view(np.uint32))


def test_whole_and_combined_plans_agree_bit_for_bit(alslib, monkeypatch):
    """The row's own length decides: the same short rows from a plan of whole rows and from a plan whose one chunked row holds
    most of the ratings (one combined launch of chunk items and whole rows) -- both hand them to the dual kernel."""
    _need_gpu()
    from cumf_als_amd import als

    f = 100
    short = tuple(n for n in LENS for _ in range(3))
    rowptr, colidx, val, table, _ = _problem(f, short)
    rng = np.random.RandomState(7)
    long_cols = rng.randint(0, TABLE_ROWS, size=4000).astype(np.int32)
    rowptr2 = np.concatenate([rowptr, [rowptr[-1] + 4000]]).astype(np.int32)
    colidx2 = np.concatenate([colidx, long_cols])
    val2 = np.concatenate([val, rng.randint(1, 6, size=4000).astype(np.float32)])
    monkeypatch.delenv("CUMF_ALS_DUAL", raising=False)
    out = []
    for rp, ci, va in ((rowptr, colidx, val), (rowptr2, colidx2, val2)):
        plan = als.Plan(rp, f, chunk=512)
        assert als.dual_rows_probe(rp, f, 512, "lu", gather_rows=TABLE_ROWS)["routed"] == sum(n <= 79 for n in short)
        x = torch.zeros((len(rp) - 1, f), device="cuda")
        als.update_fused(plan, torch.tensor(ci).cuda(), torch.tensor(va).cuda(), torch.tensor(table).cuda(), x, LAM, "lu")
        torch.cuda.synchronize()
        plan.close()
        out.append(x[: len(short)].cpu().numpy())
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
