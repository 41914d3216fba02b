"""Weighted ALS (include/cumf_weighted_capi.h) without a GPU: the numpy fp64 reference of tests/weighted_ref.py against brute
force, its two reductions (explicit and implicit), what the weights are for, the availability table, the refusals that touch
no device and the Python names."""
import ctypes as C

import numpy as np
import pytest

from tests import free_ref, implicit_ref
from tests import weighted_ref as ref

# 2^-4: (float)n * lam is exact in fp32, so the fp32 regulariser of free_ref / weighted_ref and the fp64 lam * n of implicit_ref
# are the same number and the reductions below can be held to 1e-12
LAM = 0.0625


def _case(seed=3, m=30, n=20, zero_share=0.2):
    """m x n ratings with a full row, an empty row, an empty column, stored zeros, negative ratings and weights of 0."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, n // 2, m)
    lens[0], lens[1] = n - 1, 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(n - 1, ln, replace=False)) for ln in lens]).astype(np.int32)  # column n-1: empty
    val = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0]), int(rowptr[-1]))
    wgt = rng.uniform(0.5, 4.0, len(val))
    wgt[rng.random_sample(len(val)) < zero_share] = 0.0
    return rowptr, colidx, val, wgt


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("w0", [0.0, 0.3, 1.0])
def test_sparse_loss_is_the_dense_loss(w0, reg):
    rowptr, colidx, val, wgt = _case()
    assert (wgt == 0).sum() > 10
    rng = np.random.RandomState(5)
    X, Y = 0.4 * rng.standard_normal((30, 6)), 0.4 * rng.standard_normal((20, 6))
    dense = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
    sparse = ref.sparse_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
    assert abs(dense - sparse) <= 1e-10 * abs(dense), (dense, sparse)


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("w0", [0.0, 0.3, 1.0])
def test_systems_zero_the_gradient_of_the_dense_loss(w0, reg):
    """x_u = A_u^-1 b_u zeroes dL/dx_u, the gradient written out from the m x n weight and target matrices (not from A, b)."""
    rowptr, colidx, val, wgt = _case()
    m, n, f = 30, 20, 6
    Y = 0.4 * np.random.RandomState(6).standard_normal((n, f))
    X = ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, w0, reg)
    row, col = ref._coo(rowptr, colidx)
    W, R = np.full((m, n), w0), np.zeros((m, n))
    W[row, col], R[row, col] = wgt, val
    regs = ref.reg_of(np.bincount(row, minlength=m), LAM, reg)
    grad = -2 * (W * (R - X @ Y.T)) @ Y + 2 * regs[:, None] * X
    live = np.diff(rowptr) > 0
    scale = np.abs(2 * (W * R) @ Y).max()
    assert np.abs(grad[live]).max() <= 1e-12 * scale, np.abs(grad[live]).max()
    assert (X[~live] == 0).all()
    # ... and it is a minimum: any step away raises the loss
    base = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
    rng = np.random.RandomState(7)
    for _ in range(5):
        D = 1e-3 * rng.standard_normal(X.shape) * live[:, None]
        assert ref.dense_loss(rowptr, colidx, val, wgt, X + D, Y, LAM, w0, reg) > base


def test_explicit_reduction():
    """w = 1, w0 = 0, reg lambda n: the systems of the explicit matrix-free half-iteration (tests/free_ref.py)."""
    rowptr, colidx, val, _ = _case()
    Y = 0.4 * np.random.RandomState(8).standard_normal((20, 6))
    A, b = ref.systems(rowptr, colidx, val, np.ones(len(val)), Y, LAM, 0.0, "weighted")
    A0, b0 = free_ref.systems(rowptr, colidx, val, Y, LAM)
    live = np.diff(rowptr) > 0  # (free_ref leaves an empty row's A at 0; x = 0 there either way)
    assert np.abs(A[live] - A0[live]).max() <= 1e-12 * np.abs(A0).max()
    assert np.abs(b - b0).max() <= 1e-12 * np.abs(b0).max()


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_implicit_reduction(reg):
    """w = 1 + alpha |r|, val = (r > 0), w0 = 1: the systems of implicit feedback (tests/implicit_ref.py)."""
    rowptr, colidx, val, _ = _case()
    alpha = 2.0
    Y = 0.4 * np.random.RandomState(9).standard_normal((20, 6))
    A, b = ref.systems(rowptr, colidx, (val > 0).astype(np.float64), 1 + alpha * np.abs(val), Y, LAM, 1.0, reg)
    A0, b0 = implicit_ref.systems(rowptr, colidx, val, Y, LAM, alpha, reg)
    assert np.abs(A - A0).max() <= 1e-12 * np.abs(A0).max()
    assert np.abs(b - b0).max() <= 1e-12 * np.abs(b0).max()
    X = 0.4 * np.random.RandomState(10).standard_normal((30, 6))
    R = np.full((30, 20), np.nan)
    R[ref._coo(rowptr, colidx)] = val
    want = implicit_ref.dense_loss(R, X, Y, LAM, alpha, reg)
    got = ref.dense_loss(rowptr, colidx, (val > 0).astype(np.float64), 1 + alpha * np.abs(val), X, Y, LAM, 1.0, reg)
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("w0", [0.0, 0.3, 1.0])
def test_exact_alternating_steps_never_increase_the_loss(w0, reg):
    rowptr, colidx, val, wgt = _case()
    n, f = 20, 6
    colptr, rowidx, val_t, wgt_t = ref.transpose(rowptr, colidx, val, wgt, n)
    rng = np.random.RandomState(11)
    X, Y = np.zeros((30, f)), 0.4 * rng.standard_normal((n, f))
    # the rows / columns without entries are set to 0 by a step: start them there, so that the first step cannot gain from it
    Y[np.diff(colptr) == 0] = 0
    last = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
    for _ in range(4):
        X = ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, w0, reg)
        mid = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
        Y = ref.exact_step(colptr, rowidx, val_t, wgt_t, X, LAM, w0, reg)
        new = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
        assert mid <= last * (1 + 1e-12) and new <= mid * (1 + 1e-12), (last, mid, new)
        last = new


def weights_effect(seed=0):
    """Planted rank-4 ratings of 300 x 200, three tenths of them stored (60 or 90 per row and column: with fewer than about
    40 the rank-4 factors are not identified from the low-noise half alone and neither run recovers the matrix); half of the
    stored ones carry noise of sigma = 0.1, half of sigma = 1.  Exact ALS (f = 4, reg lambda n, 15 iterations: converged) with
    w = 1 / sigma^2 and with w = 1; returns both RMSEs against the CLEAN values of held-out entries."""
    rng = np.random.RandomState(seed)
    m, n, k, lam = 300, 200, 4, 0.02
    clean = rng.standard_normal((m, k)) @ rng.standard_normal((n, k)).T
    mask = rng.random_sample((m, n)) < 0.3
    held = ~mask & (rng.random_sample((m, n)) < 0.1)
    row, col = np.nonzero(mask)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m))]).astype(np.int32)
    sigma = np.where(rng.random_sample(len(row)) < 0.5, 0.1, 1.0)
    val = clean[row, col] + sigma * rng.standard_normal(len(row))
    out = []
    for wgt in (1 / sigma ** 2, np.ones(len(row))):
        colptr, rowidx, val_t, wgt_t = ref.transpose(rowptr, col, val, wgt, n)
        Y = 0.3 * np.random.RandomState(1).standard_normal((n, k))
        for _ in range(15):
            X = ref.exact_step(rowptr, col, val, wgt, Y, lam, 0.0)
            Y = ref.exact_step(colptr, rowidx, val_t, wgt_t, X, lam, 0.0)
        out.append(float(np.sqrt((((X @ Y.T) - clean)[held] ** 2).mean())))
    return out


def test_inverse_variance_weights_lower_the_heldout_error():
    """What the weights are for: with the ratings' known noise variances as 1 / sigma^2 weights the reference recovers the
    planted matrix better than with w = 1 (measured ratio: DESIGN 4.13)."""
    weighted, plain = weights_effect()
    print(f"clean held-out RMSE: w = 1/sigma^2 {weighted:.4f}, w = 1 {plain:.4f}, ratio {weighted / plain:.3f}")
    assert weighted < plain, (weighted, plain)


def test_weighted_availability(alslib):
    from cumf_als_amd import als

    for f in range(-2, 520):
        assert alslib.cumf_weighted_available(f) == int(8 <= f <= 512 and f % 2 == 0), f
    assert als.weighted_available(8) and als.weighted_available(512) and not als.weighted_available(129)


def test_update_weighted_refuses_without_a_device(alslib, capfd):
    """A NULL plan or pointer is refused with hipErrorInvalidValue (1) and a printed reason before any device call; so are a
    negative or NaN w0 and an unknown reg mode of the loss."""
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)  # never dereferenced: the plan is NULL
    assert alslib.cumf_als_update_weighted(None, buf, buf, buf, buf, buf, buf, 0.05, 0.0, 0, 6, None) == 1
    assert "cumf_als_update_weighted" in capfd.readouterr().err
    assert alslib.cumf_als_update_weighted(None, None, None, None, None, None, None, 0.05, 0.0, 0, 6, None) == 1
    out = np.zeros(1, np.float64).ctypes.data_as(C.c_void_p)
    for f, w0, reg in ((9, 0.0, 0), (514, 0.0, 0), (64, -1.0, 0), (64, float("nan"), 0), (64, 0.0, 2)):
        capfd.readouterr()
        assert alslib.cumf_weighted_loss(buf, buf, buf, buf, buf, buf, 1, 1, f, 0.05, w0, reg, out, None) == 1, (f, w0, reg)
        assert "cumf_weighted_loss" in capfd.readouterr().err
    assert alslib.cumf_weighted_loss(buf, buf, buf, buf, buf, buf, 1, 1, 64, 0.05, 0.0, 0, None, None) == 1


def test_python_names(alslib):
    from cumf_als_amd import als

    assert callable(als.update_weighted) and callable(als.weighted_loss) and callable(als.weighted_available)
    assert issubclass(als.WeightedALSEngine, als._Engine)
    for name in ("recommend", "ranking_metrics", "heldout_ranks", "full_ranking_metrics", "loss"):
        assert callable(getattr(als.WeightedALSEngine, name))
    for w0 in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            als._check_w0(w0)
