"""The non-negative explicit block solver (als.update_block_nonneg, ALSEngine(solver="block_nonneg")) on the MI355X, fused and
segmented routes, against block Gauss-Seidel with an exact 32-wide NNLS per block (tests/nnls_ref.py) in numpy on the dense fp64
systems of tests/free_ref.py; the same recurrence with the float32 emulation of the solver's step is the error scale.  Data,
row lengths and bound form are those of tests/test_block_explicit_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests import free_ref as ref
from tests import nnls_ref
from tests.test_block_explicit_gpu import LAM, LENS, _case, _check, _dev

pytestmark = pytest.mark.gpu
LIVE = np.asarray(LENS) > 0
# _check's constant: twice the largest measured ratio (4.54: f = 32, one sweep), rounded up.  The ratios fall with f (510: 1.04):
# at small f numpy's c = (b - A x) + H x cancels one rounded product exactly, the kernel's g and H x round apart.
C = 10.0


def nonneg_ref(A, b, x0, sweeps, lens, B=32):
    """`sweeps` sweeps of block Gauss-Seidel under x >= 0 from x0 in the dtype of A, each block step the NNLS in z with
    c = rhs + H x[pi] from the passive set {x[pi] > 0}; rows without entries get 0.  Returns (x, eliminations)."""
    solve = nnls_ref.nnls_trace_fp32 if A.dtype == np.float32 else nnls_ref.nnls_trace
    x, elims = x0.astype(A.dtype), 0
    for u in np.flatnonzero(np.asarray(lens) > 0):
        for c in [c for _ in range(sweeps) for c in range(0, x.shape[1], B)]:
            H = A[u, c:c + B, c:c + B]
            t = solve(H, (b[u] - A[u] @ x[u])[c:c + B] + H @ x[u, c:c + B], F0=x[u, c:c + B] > 0)
            x[u, c:c + B], elims = t.x, elims + t.factorisations
    x[np.asarray(lens) == 0] = 0
    return x, elims


@functools.lru_cache(maxsize=4)
def _refs(f, sweeps):
    _, _, _, _, x0, (A64, b64), (A32, b32) = _case(f)
    x64, elims = nonneg_ref(A64, b64, x0, sweeps, LENS)
    return x64, nonneg_ref(A32, b32, x0, sweeps, LENS)[0], elims


def _update(f, sweeps, route="auto", cuts=None, chunk=0):
    from cumf_als_amd import als

    rowptr, colidx, val, Y, x0 = _case(f)[:5]
    x, stats, cuts = _dev(x0.copy()), torch.zeros(2, dtype=torch.int64, device="cuda"), cuts or [0, len(LENS)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(rowptr, f, lo, hi, chunk)
        als.update_block_nonneg(plan, _dev(colidx), _dev(val), _dev(Y), x, LAM, sweeps, route, stats)
        torch.cuda.synchronize()
        fused = route == "auto" and min(LENS[lo:hi]) <= 2048  # the fused launches come last
        assert ("block_fused_kernel" if fused else "block_row_free_kernel") in als.last_kernel_name()
        plan.close()
    return x.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("route", ["auto", "segmented"])
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("f", [8, 32, 34, 66, 130, 510])
def test_block_nonneg_step_parity(alslib, f, sweeps, route):
    x64, x32, _ = _refs(f, sweeps)
    # a solver that ignores the constraint cannot pass: every live reference row has an exact zero and a positive coordinate
    assert ((x64[LIVE] == 0).any(1) & (x64[LIVE] > 0).any(1)).all()
    # two plans: the rows of at most 2048 entries (the fused kernel alone under "auto") and the longer ones
    x, stats = _update(f, sweeps, route, cuts=[0, LENS.index(2049), len(LENS)])
    assert x.min() >= 0 and stats[0] == 0, (x.min(), stats)
    _check(f"nonneg f={f} sweeps={sweeps} {route}", x, x64, x32, LIVE, C)


@pytest.mark.parametrize("f", [8, 32])
def test_one_block_is_the_exact_nnls(alslib, f):
    (A64, b64), (A32, b32) = _case(f)[5:]
    x64, x32 = np.zeros_like(b64), np.zeros_like(b32)
    for u in np.flatnonzero(LIVE):
        x64[u], x32[u] = nnls_ref.nnls(A64[u], b64[u])[0], nnls_ref.nnls_trace_fp32(A32[u], b32[u]).x
    x, _ = _update(f, 1)
    assert x.min() >= 0
    _check(f"nonneg exact f={f}", x, x64, x32, LIVE, C)


def test_block_nonneg_bits(alslib):
    """The fused and the segmented route, three plans and the plan's chunks: bit-identical factors and statistics."""
    f, rows = 66, len(LENS)
    want, stats = _update(f, 2)  # stats[1] is printed, not compared: a sign test within tolerance may differ from fp64's
    print(f"nonneg eliminations f={f} sweeps=2: hip {int(stats[1])} fp64 trace {_refs(f, 2)[2]}")
    assert stats[0] == 0 and stats[1] > 0, stats
    for kw in ({"route": "segmented"}, {"cuts": [0, rows // 3, 2 * rows // 3, rows]}, {"chunk": 1000},
               {"cuts": [0, 7, rows], "chunk": 1000, "route": "segmented"}):
        x, st = _update(f, 2, **kw)
        assert np.array_equal(x, want) and np.array_equal(st, stats), kw


def test_block_nonneg_engine(alslib):
    """Two iterations of ALSEngine(solver="block_nonneg") against the same recurrence in numpy on both sides."""
    from cumf_als_amd import als, datagen

    f = 66
    r = datagen.synth_ratings(300, 200, 6000, 100, seed=5)
    for kw in ({"f": 514}, {"cg_iters": 0}, {"nonnegative": True}):
        with pytest.raises(ValueError):
            als.ALSEngine(r.to("cuda"), **{"f": f, "lambda_": LAM, "solver": "block_nonneg", **kw})
    for make in (lambda: als.WeightedALSEngine(r.to("cuda"), torch.ones(r.nnz, device="cuda"), f, LAM, solver="block_nonneg"),
                 lambda: als.BiasedALSEngine(r.to("cuda"), f, LAM, solver="block_nonneg")):
        with pytest.raises((ValueError, TypeError)):  # the weighted engine has no solver argument at all
            make()
    e = als.ALSEngine(r.to("cuda"), f, LAM, solver="block_nonneg", cg_iters=1, x_batch=3, chunk=1000)
    e.init_factors(seed=1)
    d = r.numpy()
    csr, csc = [(d[k + "_indptr"], d[k + "_indices"], d[k + "_data"]) for k in ("csr", "csc")]
    out = {}
    for dtype in (np.float64, np.float32):
        X, T = e.XT.cpu().numpy().astype(dtype), e.thetaT.cpu().numpy().astype(dtype)
        for _ in range(2):
            X = nonneg_ref(*ref.systems(*csr, T, LAM, dtype), X, 1, np.diff(csr[0]))[0]
            T = nonneg_ref(*ref.systems(*csc, X, LAM, dtype), T, 1, np.diff(csc[0]))[0]
        out[dtype] = X, T
    e.iterate(2)
    assert e.nnls_stats[0].item() == 0 and e.nnls_stats[1].item() > 0
    for name, x, x64, x32 in zip(("X", "Theta"), (e.XT.cpu().numpy(), e.thetaT.cpu().numpy()), out[np.float64], out[np.float32]):
        assert x.min() >= 0, name
        _check(f"nonneg engine {name}", x, x64, x32, np.diff((csr if name == "X" else csc)[0]) > 0, C)
    e.close()
