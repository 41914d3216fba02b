"""The sixteen-pivot steps of the one-wave LU (lu_wave_blocked16: the default at NB = 7, f = 96 .. 111) against the fp64
oracle and against the four-pivot panels (CUMF_ALS_LU16=0) of the same process on the same rows.  f = 64 (NB = 5) and f = 80
(NB = 6) keep the four-pivot panels, and so does the dual kernel of the short rows at f = 100 -- the scheme was measured
slower at five blocks -- and there the switch must change nothing.

Bound: both schemes accumulate in fp32 from exactly split operands and differ in the order of summation only, so the new
scheme's largest per-row deviation from the fp64 oracle may be at most twice the four-pivot scheme's, measured in the same
run; and it stays within the project's LU tolerance, 1e-4 of the row's scale (tests/test_gpu_parity.py).  The ill-conditioned
systems (condition numbers up to 1e6) have no absolute bound in the project -- there the 1e-4 is asserted where the four-pivot
scheme meets it itself.  Fused train SSE: 2e-5 relative against the RMSE kernel
(test_fused_train_sse_matches_the_rmse_kernel)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

TABLE_ROWS = 400
LAM = 0.05
WAVE_LENS = (80, 81, 96, 97, 128, 300)        # f = 96, 100: the first lengths past the dual route, the stage seams, a long row
SMALL_LENS = (1, 16, 33, 64, 65, 96, 97, 300)  # f = 64, 80: every row is the wave kernel's
DUAL_LENS = (1, 16, 17, 63, 64, 65, 79)       # run-time size n' = 64 .. 79 and the padded pivots lambda n


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


@functools.lru_cache(maxsize=None)
def _problem(f, lens):
    """(rowptr, colidx, val, table, x64): rows of the given lengths (distinct table rows per row, ratings 1 .. 5) and the
    fp64 oracle half-iteration, computed once per shape."""
    from oracle import pyoracle

    pyoracle.build()
    rng = np.random.RandomState(1)
    table = (0.2 * rng.random_sample((TABLE_ROWS, f))).astype(np.float32)
    rng = np.random.RandomState(2)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([rng.choice(TABLE_ROWS, n, replace=False) for n in lens] + [[]]).astype(np.int32)
    val = rng.randint(1, 6, size=len(colidx)).astype(np.float32)
    x64 = np.zeros((len(lens), f), np.float32)  # the oracle computes in fp64 and stores fp32
    pyoracle.half_iteration(rowptr, colidx, val, table, x64, f, LAM, solver="lu", dtype=np.float64)
    for a in (rowptr, colidx, val, table, x64):
        a.setflags(write=False)
    return rowptr, colidx, val, table, x64


def _run(f, rowptr, colidx, val, table, lam=LAM, chunk=0):
    """One LU half-iteration on the GPU: the factors and the name of the route's kernel."""
    from cumf_als_amd import als

    rows = len(rowptr) - 1
    x = torch.zeros((rows, f), device="cuda")
    plan = als.Plan(rowptr, f, chunk=chunk)
    chunked = plan.n_multi_rows
    als.update_fused(plan, torch.tensor(colidx).cuda(), torch.tensor(val).cuda(), torch.tensor(table).cuda(), x, lam, "lu")
    torch.cuda.synchronize()
    plan.close()
    return x.cpu().numpy(), als.last_kernel_name(), chunked


def _both_schemes(monkeypatch, *args, **kw):
    monkeypatch.delenv("CUMF_ALS_LU16", raising=False)
    new = _run(*args, **kw)
    monkeypatch.setenv("CUMF_ALS_LU16", "0")
    four = _run(*args, **kw)
    monkeypatch.delenv("CUMF_ALS_LU16")
    return new, four


def _row_dev(x, x64):
    return np.abs(x - x64).max(axis=1) / np.abs(x64).max(axis=1)


def _check(label, lens, xn, xf, x64):
    assert np.isfinite(xn).all() and np.isfinite(xf).all()
    dn, df = _row_dev(xn, x64), _row_dev(xf, x64)
    print(f"{label}: max per-row relative deviation from the fp64 oracle: sixteen-pivot {dn.max():.3e}  "
          f"four-pivot {df.max():.3e}")
    for n in sorted(set(lens)):
        sel = np.array(lens) == n
        print(f"  n={n:3d}: sixteen-pivot {dn[sel].max():.3e}  four-pivot {df[sel].max():.3e}")
    assert dn.max() <= 1e-4, dn.max()
    assert dn.max() <= 2.0 * df.max(), (dn.max(), df.max())


@pytest.mark.parametrize("f,lens", [(100, WAVE_LENS), (96, WAVE_LENS), (64, SMALL_LENS), (80, SMALL_LENS)])
def test_whole_rows_against_the_fp64_oracle_and_the_four_pivot_scheme(alslib, monkeypatch, f, lens):
    _need_gpu()
    lens3 = tuple(n for n in lens for _ in range(3))
    rowptr, colidx, val, table, x64 = _problem(f, lens3)
    (xn, kn, _), (xf, kf, _) = _both_schemes(monkeypatch, f, rowptr, colidx, val, table)
    if f >= 96:
        assert "als_wave_kernel<" in kn and "als_wave_kernel_p4<" in kf, (kn, kf)  # the switch routes
        assert not np.array_equal(xn.view(np.uint32), xf.view(np.uint32))          # ... to another elimination
    else:
        assert kn == kf and "als_wave_kernel<" in kn and np.array_equal(xn.view(np.uint32), xf.view(np.uint32)), (kn, kf)
    _check(f"whole rows f={f}", lens3, xn, xf, x64)


def test_chunked_rows_and_a_row_without_ratings(alslib, monkeypatch):
    """A plan whose chunk is forced small: the rows of 300 ratings go through the reduce path, the others are solved in the
    kernel (one combined launch); the row without ratings gives the four-pivot scheme's NaN pattern."""
    _need_gpu()
    f = 100
    lens3 = tuple(n for n in WAVE_LENS for _ in range(3)) + (0,)
    rowptr, colidx, val, table, x64 = _problem(f, lens3)
    (xn, _, chunked), (xf, _, _) = _both_schemes(monkeypatch, f, rowptr, colidx, val, table, chunk=128)
    assert chunked == 3
    assert np.array_equal(np.isnan(xn), np.isnan(xf)) and np.isnan(xn[-1]).all() and np.isfinite(xn[:-1]).all()
    _check("chunked plan f=100", lens3[:-1], xn[:-1], xf[:-1], x64[:-1])


def test_dual_kernel(alslib, monkeypatch):
    _need_gpu()
    from cumf_als_amd import als

    f = 100
    lens3 = tuple(n for n in DUAL_LENS for _ in range(3))
    rowptr, colidx, val, table, x64 = _problem(f, lens3)
    plan = als.Plan(rowptr, f)
    routed = als.dual_rows_probe(rowptr, f, plan.chunk, "lu", gather_rows=TABLE_ROWS)["routed"]
    plan.close()
    assert routed == len(lens3)
    (xn, _, _), (xf, _, _) = _both_schemes(monkeypatch, f, rowptr, colidx, val, table)
    assert np.array_equal(xn.view(np.uint32), xf.view(np.uint32))  # lu_wave_blocked<5> keeps the four-pivot panels
    _check("dual kernel f=100", lens3, xn, xf, x64)


@functools.lru_cache(maxsize=None)
def _ill_conditioned(f, lam):
    """The systems of test_fused_lu_on_ill_conditioned_systems (tests/test_gpu_parity.py): ~400 ratings per row, factors of
    mixed signs, condition number ~ |x|^2 / lambda."""
    from cumf_als_amd import datagen
    from oracle import pyoracle

    pyoracle.build()
    r = datagen.synth_ratings(400, 3000, 160000, 600, seed=21)
    d = r.numpy()
    rng = np.random.RandomState(5)
    theta = (0.2 * rng.random_sample((r.n, f))).astype(np.float32) - 0.08
    x64 = np.zeros((r.m, f), np.float32)
    x64 = pyoracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x64, f, lam, solver="lu",
                                  dtype=np.float64)
    return d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x64


@pytest.mark.parametrize("f", [100, 64])
@pytest.mark.parametrize("lam", [0.05, 1e-3, 1e-5])
def test_ill_conditioned_systems(alslib, monkeypatch, f, lam):
    _need_gpu()
    rowptr, colidx, val, theta, x64 = _ill_conditioned(f, lam)
    (xn, _, _), (xf, _, _) = _both_schemes(monkeypatch, f, rowptr, colidx, val, theta, lam=lam)
    fin = np.isfinite(x64).all(1)
    assert np.array_equal(np.isfinite(xn).all(1), fin) and np.array_equal(np.isfinite(xf).all(1), fin)
    dn, df = _row_dev(xn[fin], x64[fin]), _row_dev(xf[fin], x64[fin])
    stats = lambda v: (float(np.median(v)), float(np.quantile(v, 0.99)), float(v.max()))
    print(f"ill-conditioned LU f={f} lambda={lam}: per-row relative |x - x64| (median, q99, max): sixteen-pivot {stats(dn)}  "
          f"four-pivot {stats(df)}")
    assert dn.max() <= 2.0 * df.max(), (stats(dn), stats(df))
    if df.max() <= 1e-4:
        assert dn.max() <= 1e-4, stats(dn)


def test_fused_train_sse(alslib, monkeypatch):
    _need_gpu()
    from cumf_als_amd import als, datagen

    f = 100
    monkeypatch.delenv("CUMF_ALS_LU16", raising=False)
    r = datagen.synth_ratings(900, 700, 60000, 500, seed=5)
    rg = r.to("cuda")
    eng = als.ALSEngine(rg, f, 0.05, solver="lu")
    rng = np.random.RandomState(3)
    eng.init_factors((0.2 * rng.random_sample((r.n, f))).astype(np.float32))
    for it in range(2):
        eng.update_x()
        fused = eng.update_theta_with_train_sse()
        assert fused is not None
        torch.cuda.synchronize()
        assert "als_wave_kernel<7, 1, 100" in als.last_kernel_name()
        kern = float(als.sse(rg.csr_data, rg.coo_row, rg.csr_indices, eng.thetaT, eng.XT).item())
        got = float(fused.item())
        print(f"fused train SSE f={f} lu iter {it}: fused {got:.6f} kernel {kern:.6f}  rel {abs(got - kern) / kern:.2e}")
        assert abs(got - kern) <= 2e-5 * kern, (got, kern)
