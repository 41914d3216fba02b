"""The iALS++ block solver of implicit feedback (solver "block", CUMF_SOLVER_BLOCK) on the MI355X, against the same block
Gauss-Seidel recurrence in numpy on the dense fp64 systems of tests/implicit_ref.py; the recurrence in float32 is the error scale."""
import functools

import numpy as np
import pytest
import torch

from tests import implicit_ref as ref

pytestmark = pytest.mark.gpu

LAM = 0.05
# the MFMA K tail (3, 4, 5), the four groups in flight (15, 16, 17), the opening pass's reductions (7, 8, 9), the 64-entry index
# load (63, 64, 65, 128), the segment cut (2047, 2048, 2049) and three segments (4097)
LENS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 2047, 2048, 2049, 4097]
N_COLS = 4200


def block_ref(A, b, x0, sweeps, lens, B=32):
    """`sweeps` sweeps of exact block Gauss-Seidel on A x = b from x0, in the dtype of A; rows without entries get 0."""
    x = x0.astype(A.dtype)
    for u in range(len(x)):
        for c in [c for _ in range(sweeps) for c in range(0, x.shape[1], B)]:
            x[u, c:c + B] += np.linalg.solve(A[u, c:c + B, c:c + B], (b[u] - A[u] @ x[u])[c:c + B])
    x[np.asarray(lens) == 0] = 0
    return x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=2)
def _case(f, alpha, reg):
    rng = np.random.RandomState(7)
    rowptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(N_COLS, ln, replace=False)) for ln in LENS]).astype(np.int32)
    val = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0], np.float32), int(rowptr[-1]))
    Y = (0.3 * np.random.RandomState(3).standard_normal((N_COLS, f))).astype(np.float32)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(LENS), f))).astype(np.float32)
    sys64 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
    sys32 = ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg, dtype=np.float32)
    return rowptr, colidx, val, Y, x0, sys64, sys32


def _update(rowptr, colidx, val, Y, x0, f, alpha, reg, sweeps, cuts=None, chunk=0):
    from cumf_als_amd import als

    Yg, x = _dev(Y), _dev(x0.copy())
    G = als.implicit_gram(Yg)
    cuts = cuts or [0, len(rowptr) - 1]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(rowptr, f, lo, hi, chunk)
        als.update_implicit(plan, _dev(colidx), _dev(val), Yg, G, x, LAM, alpha, reg, "block", sweeps)
        torch.cuda.synchronize()
        assert "block_row_kernel" in als.last_kernel_name()
        plan.close()
    return x.cpu().numpy()


def _stats(v):
    return float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max())


def _check(tag, x, x64, x32, c=2.0):
    """Per row the max-norm distance to the fp64 reference; its median / q90 / max over the rows within c x those of the
    float32 reference + 1e-5 of the factors' scale (the bound form of tests/test_implicit_matfree_gpu.py)."""
    live = np.asarray(LENS) > 0
    assert (x[~live] == 0).all(), tag
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1)[live], np.abs(x32 - x64).max(1)[live]
    print(f"implicit block {tag}: hip {_stats(e_h)} numpy32 {_stats(e_o)} ratios "
          f"{[round(h / o, 3) for h, o in zip(_stats(e_h), _stats(e_o))]}")
    for sh, so in zip(_stats(e_h), _stats(e_o)):
        assert so <= c * so + 1e-5 * scale  # the float32 reference alone meets the bound
        assert sh <= c * so + 1e-5 * scale, (tag, _stats(e_h), _stats(e_o))


@pytest.mark.parametrize("alpha,reg", [(1.0, "weighted"), (40.0, "plain")])
@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("f", [8, 32, 34, 66, 130, 510])
def test_block_step_parity(alslib, f, sweeps, alpha, reg):
    rowptr, colidx, val, Y, x0, (A64, b64), (A32, b32) = _case(f, alpha, reg)
    x = _update(rowptr, colidx, val, Y, x0, f, alpha, reg, sweeps)
    _check(f"f={f} sweeps={sweeps} alpha={alpha} {reg}", x, block_ref(A64, b64, x0, sweeps, LENS),
           block_ref(A32, b32, x0, sweeps, LENS))


@pytest.mark.parametrize("f", [8, 32])
def test_one_block_is_the_exact_solve(alslib, f):
    rowptr, colidx, val, Y, x0, (A64, b64), (A32, b32) = _case(f, 40.0, "plain")
    x = _update(rowptr, colidx, val, Y, x0, f, 40.0, "plain", 1)
    live = np.asarray(LENS) > 0
    x64, x32 = np.zeros_like(b64), np.zeros_like(b32)
    x64[live], x32[live] = np.linalg.solve(A64[live], b64[live][..., None])[..., 0], np.linalg.solve(A32[live], b32[live][..., None])[..., 0]
    _check(f"exact f={f}", x, x64, x32)


def test_block_bits(alslib):
    """The same half-iteration twice, through three plans and with the plan's chunks: bit-identical."""
    f = 66
    rowptr, colidx, val, Y, x0, _, _ = _case(f, 40.0, "plain")
    rows = len(LENS)
    want = _update(rowptr, colidx, val, Y, x0, f, 40.0, "plain", 2)
    for kw in ({}, {"cuts": [0, rows // 3, 2 * rows // 3, rows]}, {"chunk": 1000}, {"cuts": [0, 7, rows], "chunk": 1000}):
        assert np.array_equal(_update(rowptr, colidx, val, Y, x0, f, 40.0, "plain", 2, **kw), want), kw


def test_block_engine(alslib):
    """Two iterations of ImplicitALSEngine(solver="block") against the same recurrence in numpy on both sides (G and the
    systems in fp64; in float32 for the error scale)."""
    from cumf_als_amd import als, datagen

    f, alpha = 66, 40.0
    r = datagen.synth_ratings(300, 200, 6000, 100, seed=5)
    with pytest.raises(ValueError):
        als.ImplicitALSEngine(r.to("cuda"), 514, LAM, alpha, solver="block")
    e = als.ImplicitALSEngine(r.to("cuda"), f, LAM, alpha, solver="block", cg_iters=1, x_batch=3, chunk=1000)
    e.init_factors(seed=1)
    d = r.numpy()
    csr, csc = [(d[k + "_indptr"], d[k + "_indices"], d[k + "_data"]) for k in ("csr", "csc")]
    out = {}
    for dtype in (np.float64, np.float32):
        X, T = e.XT.cpu().numpy().astype(dtype), e.thetaT.cpu().numpy().astype(dtype)
        for _ in range(2):
            X = block_ref(*ref.systems(*csr, T, LAM, alpha, dtype=dtype), X, 1, np.diff(csr[0]))
            T = block_ref(*ref.systems(*csc, X, LAM, alpha, dtype=dtype), T, 1, np.diff(csc[0]))
        out[dtype] = X, T
    e.iterate(2)
    got, want = e.loss(), ref.sparse_loss(*csr, *out[np.float64], LAM, alpha)
    for name, x, x64, x32 in zip(("X", "Theta"), (e.XT.cpu().numpy(), e.thetaT.cpu().numpy()), out[np.float64], out[np.float32]):
        scale = np.abs(x64).max()
        e_h, e_o = np.abs(x - x64).max(1), np.abs(x32 - x64).max(1)
        print(f"implicit block engine {name}: hip {_stats(e_h)} numpy32 {_stats(e_o)}")
        for sh, so in zip(_stats(e_h), _stats(e_o)):
            assert sh <= 2.0 * so + 1e-5 * scale, (name, _stats(e_h), _stats(e_o))
    print(f"implicit block engine loss: hip {got!r} reference {want!r} relative {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    e.close()
