"""The explicit block solver (als.update_block, ALSEngine(solver="block")) on the MI355X, fused and segmented routes, against
the block Gauss-Seidel recurrence in numpy on the dense fp64 systems of tests/free_ref.py; the recurrence in float32 is the
error scale."""
import functools

import numpy as np
import pytest
import torch

from tests import free_ref as ref

pytestmark = pytest.mark.gpu

LAM = 0.05
# the MFMA K tail (3, 4, 5), the four groups in flight (15, 16, 17), the opening pass's reductions (7, 8, 9), the 64-entry index
# load (63, 64, 65, 128), the capacity classes of the fused kernel (959, 960, 961), the fused / segmented seam (2047, 2048,
# 2049) and three segments (4097)
LENS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 959, 960, 961, 2047, 2048, 2049, 4097]
N_COLS = 4200


def block_ref(A, b, x0, sweeps, lens, B=32):
    """`sweeps` sweeps of exact block Gauss-Seidel on A x = b from x0, in the dtype of A; rows without entries get 0."""
    x = x0.astype(A.dtype)
    for u in np.flatnonzero(np.asarray(lens) > 0):
        for c in [c for _ in range(sweeps) for c in range(0, x.shape[1], B)]:
            x[u, c:c + B] += np.linalg.solve(A[u, c:c + B, c:c + B], (b[u] - A[u] @ x[u])[c:c + B])
    x[np.asarray(lens) == 0] = 0
    return x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=2)
def _case(f):
    rng = np.random.RandomState(7)
    rowptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(N_COLS, ln, replace=False)) for ln in LENS]).astype(np.int32)
    val = rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 4.0, 5.0], np.float32), int(rowptr[-1]))
    Y = (0.3 * np.random.RandomState(3).standard_normal((N_COLS, f))).astype(np.float32)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(LENS), f))).astype(np.float32)
    return rowptr, colidx, val, Y, x0, ref.systems(rowptr, colidx, val, Y, LAM), ref.systems(rowptr, colidx, val, Y, LAM, np.float32)


def _update(rowptr, colidx, val, Y, x0, f, sweeps, route="auto", cuts=None, chunk=0):
    from cumf_als_amd import als

    Yg, x = _dev(Y), _dev(x0.copy())
    cuts = cuts or [0, len(rowptr) - 1]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(rowptr, f, lo, hi, chunk)
        als.update_block(plan, _dev(colidx), _dev(val), Yg, x, LAM, sweeps, route)
        torch.cuda.synchronize()
        # the fused launches come last; a plan without a row of at most 2048 entries has none
        fused = route == "auto" and min(LENS[lo:hi]) <= 2048
        assert ("block_fused_kernel" if fused else "block_row_free_kernel") in als.last_kernel_name()
        plan.close()
    return x.cpu().numpy()


def _stats(v):
    return float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max())


def _check(tag, x, x64, x32, live, c=2.0):
    """Per row the max-norm distance to the fp64 reference; its median / q90 / max over the live rows within c x those of the
    float32 reference + 1e-5 of the factors' scale (the bound form of tests/test_implicit_block_gpu.py)."""
    assert (x[~live] == 0).all(), tag
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1)[live], np.abs(x32 - x64).max(1)[live]
    print(f"explicit block {tag}: hip {_stats(e_h)} numpy32 {_stats(e_o)} ratios "
          f"{[round(h / o, 3) for h, o in zip(_stats(e_h), _stats(e_o))]}")
    for sh, so in zip(_stats(e_h), _stats(e_o)):
        assert sh <= c * so + 1e-5 * scale, (tag, _stats(e_h), _stats(e_o))


@pytest.mark.parametrize("f", [8, 32, 34, 66, 130, 510])
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("route", ["auto", "segmented"])
def test_block_step_parity(alslib, f, sweeps, route):
    rowptr, colidx, val, Y, x0, (A64, b64), (A32, b32) = _case(f)
    # two plans: the rows of at most 2048 entries (the fused kernel alone under "auto") and the longer ones
    x = _update(rowptr, colidx, val, Y, x0, f, sweeps, route, cuts=[0, LENS.index(2049), len(LENS)])
    _check(f"f={f} sweeps={sweeps} {route}", x, block_ref(A64, b64, x0, sweeps, LENS), block_ref(A32, b32, x0, sweeps, LENS),
           np.asarray(LENS) > 0)


@pytest.mark.parametrize("f", [8, 32])
def test_one_block_is_the_exact_solve(alslib, f):
    rowptr, colidx, val, Y, x0, (A64, b64), (A32, b32) = _case(f)
    x = _update(rowptr, colidx, val, Y, x0, f, 1)
    live = np.asarray(LENS) > 0
    x64, x32 = np.zeros_like(b64), np.zeros_like(b32)
    x64[live], x32[live] = np.linalg.solve(A64[live], b64[live][..., None])[..., 0], np.linalg.solve(A32[live], b32[live][..., None])[..., 0]
    _check(f"exact f={f}", x, x64, x32, live)


def test_block_bits(alslib):
    """The fused and the segmented route, three plans and the plan's chunks: bit-identical."""
    f = 66
    rowptr, colidx, val, Y, x0, _, _ = _case(f)
    rows = len(LENS)
    want = _update(rowptr, colidx, val, Y, x0, f, 2)
    for kw in ({"route": "segmented"}, {"cuts": [0, rows // 3, 2 * rows // 3, rows]}, {"chunk": 1000},
               {"cuts": [0, 7, rows], "chunk": 1000, "route": "segmented"}):
        assert np.array_equal(_update(rowptr, colidx, val, Y, x0, f, 2, **kw), want), kw


def test_block_engine(alslib):
    """Two iterations of ALSEngine(solver="block") against the same recurrence in numpy on both sides, and the train RMSE
    against that of the fp64 reference factors."""
    from cumf_als_amd import als, datagen

    f = 66
    r = datagen.synth_ratings(300, 200, 6000, 100, seed=5)
    for kw in ({"f": 514}, {"nonnegative": True}, {"cg_iters": 0}):
        with pytest.raises(ValueError):
            als.ALSEngine(r.to("cuda"), **{"f": f, "lambda_": LAM, "solver": "block", **kw})
    e = als.ALSEngine(r.to("cuda"), f, LAM, solver="block", cg_iters=1, x_batch=3, chunk=1000)
    e.init_factors(seed=1)
    d = r.numpy()
    csr, csc = [(d[k + "_indptr"], d[k + "_indices"], d[k + "_data"]) for k in ("csr", "csc")]
    out = {}
    for dtype in (np.float64, np.float32):
        X, T = e.XT.cpu().numpy().astype(dtype), e.thetaT.cpu().numpy().astype(dtype)
        for _ in range(2):
            X = block_ref(*ref.systems(*csr, T, LAM, dtype), X, 1, np.diff(csr[0]))
            T = block_ref(*ref.systems(*csc, X, LAM, dtype), T, 1, np.diff(csc[0]))
        out[dtype] = X, T
    e.iterate(2)
    for name, x, x64, x32 in zip(("X", "Theta"), (e.XT.cpu().numpy(), e.thetaT.cpu().numpy()), out[np.float64], out[np.float32]):
        _check(f"engine {name}", x, x64, x32, np.diff((csr if name == "X" else csc)[0]) > 0)
    X, T = out[np.float64]
    rows = np.repeat(np.arange(len(X)), np.diff(csr[0]))
    want = float(np.sqrt(np.mean((csr[2] - np.einsum("ef,ef->e", X[rows], T[csr[1]])) ** 2)))
    got = e.rmse()[0]
    print(f"explicit block engine train rmse: hip {got!r} reference {want!r} relative {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-5 * want, (got, want)
    e.close()
