"""Weighted ALS with rank-one weights a_u c_i on the unstored entries (include/cumf_weighted_capi.h) without a GPU: the numpy
fp64 reference of tests/weighted_rank1_ref.py against brute force, its reduction to tests/weighted_ref.py (a = w0, c = 1), the
refusals that touch no device and the Python names."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import weighted_rank1_ref as ref
from tests import weighted_ref
from tests.test_weighted import LAM, _case

M, N, F = 30, 20, 4


def _rank1(seed=17):
    """a over the rows from uniform [0, 1], c over the columns from uniform [0, 2], a tenth of each 0."""
    rng = np.random.RandomState(seed)
    a, c = rng.uniform(0.0, 1.0, M), rng.uniform(0.0, 2.0, N)
    a[rng.choice(M, M // 10, replace=False)] = 0.0
    c[rng.choice(N, N // 10, replace=False)] = 0.0
    return a, c


def _data():
    rowptr, colidx, val, wgt = _case(m=M, n=N, zero_share=0.1)
    assert (wgt == 0).any()
    return rowptr, colidx, val, wgt


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_sparse_loss_is_the_dense_loss(reg):
    rowptr, colidx, val, wgt = _data()
    a, c = _rank1()
    assert (a == 0).sum() == 3 and (c == 0).sum() == 2
    rng = np.random.RandomState(5)
    X, Y = 0.4 * rng.standard_normal((M, F)), 0.4 * rng.standard_normal((N, F))
    dense = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
    sparse = ref.sparse_loss(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
    assert abs(dense - sparse) <= 1e-12 * abs(dense), (dense, sparse)


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_exact_step_zeroes_the_gradient_of_the_dense_loss(reg):
    """x_u = A_u^-1 b_u zeroes dL/dx_u, the gradient written out from the m x n weight and target matrices (not from A, b)."""
    rowptr, colidx, val, wgt = _data()
    a, c = _rank1()
    Y = 0.4 * np.random.RandomState(6).standard_normal((N, F))
    X = ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, a, c, reg)
    row, col = weighted_ref._coo(rowptr, colidx)
    W, R = np.outer(a, c), np.zeros((M, N))
    W[row, col], R[row, col] = wgt, val
    regs = weighted_ref.reg_of(np.bincount(row, minlength=M), LAM, reg)
    grad = -2 * (W * (R - X @ Y.T)) @ Y + 2 * regs[:, None] * X
    live = np.diff(rowptr) > 0
    scale = np.abs(2 * (W * R) @ Y).max()
    assert np.abs(grad[live]).max() <= 1e-12 * scale, np.abs(grad[live]).max()
    assert (X[~live] == 0).all()
    # the other side: own and gather change places
    colptr, rowidx, val_t, wgt_t = weighted_ref.transpose(rowptr, colidx, val, wgt, N)
    Xf = 0.4 * np.random.RandomState(7).standard_normal((M, F))
    Yn = ref.exact_step(colptr, rowidx, val_t, wgt_t, Xf, LAM, c, a, reg)
    regs_t = weighted_ref.reg_of(np.bincount(col, minlength=N), LAM, reg)
    grad_t = -2 * (W * (R - Xf @ Yn.T)).T @ Xf + 2 * regs_t[:, None] * Yn
    live_t = np.diff(colptr) > 0
    assert np.abs(grad_t[live_t]).max() <= 1e-12 * np.abs(2 * (W * R).T @ Xf).max()


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_exact_alternating_steps_never_increase_the_loss(reg):
    rowptr, colidx, val, wgt = _data()
    a, c = _rank1()
    colptr, rowidx, val_t, wgt_t = weighted_ref.transpose(rowptr, colidx, val, wgt, N)
    rng = np.random.RandomState(11)
    X, Y = np.zeros((M, F)), 0.4 * rng.standard_normal((N, F))
    Y[np.diff(colptr) == 0] = 0  # a step sets the columns without entries to 0: start them there
    last = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
    for _ in range(4):
        X = ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, a, c, reg)
        mid = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
        Y = ref.exact_step(colptr, rowidx, val_t, wgt_t, X, LAM, c, a, reg)
        new = ref.dense_loss(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
        assert mid <= last * (1 + 1e-12) and new <= mid * (1 + 1e-12), (last, mid, new)
        last = new


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("w0", [0.0, 0.3, 1.0])
def test_reduction_to_one_scalar(w0, reg):
    """a = w0, c = 1: every reference function is its counterpart of tests/weighted_ref.py."""
    rowptr, colidx, val, wgt = _data()
    a, c = np.full(M, w0), np.ones(N)
    rng = np.random.RandomState(8)
    X, Y = 0.4 * rng.standard_normal((M, F)), 0.4 * rng.standard_normal((N, F))
    A, b = ref.systems(rowptr, colidx, val, wgt, Y, LAM, a, c, reg)
    A0, b0 = weighted_ref.systems(rowptr, colidx, val, wgt, Y, LAM, w0, reg)
    assert np.abs(A - A0).max() <= 1e-12 * np.abs(A0).max() and np.abs(b - b0).max() <= 1e-12 * np.abs(b0).max()
    for fn in ("dense_loss", "sparse_loss"):
        got = getattr(ref, fn)(rowptr, colidx, val, wgt, X, Y, LAM, a, c, reg)
        want = getattr(weighted_ref, fn)(rowptr, colidx, val, wgt, X, Y, LAM, w0, reg)
        assert abs(got - want) <= 1e-12 * abs(want), (fn, got, want)
    got = ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, a, c, reg)
    want = weighted_ref.exact_step(rowptr, colidx, val, wgt, Y, LAM, w0, reg)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_rank1_refuses_without_a_device(alslib, capfd):
    """A NULL plan or pointer is refused with hipErrorInvalidValue (1) and a printed reason before any device call; so are a
    bad f or reg mode of the Gram and of the objective."""
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)  # never dereferenced
    assert alslib.cumf_als_update_weighted_rank1(None, buf, buf, buf, buf, buf, buf, buf, buf, 0.05, 0, 6, None) == 1
    assert "cumf_als_update_weighted_rank1" in capfd.readouterr().err
    assert alslib.cumf_als_update_weighted_rank1(None, None, None, None, None, None, None, None, None, 0.05, 0, 6, None) == 1
    out = np.zeros(1, np.float64).ctypes.data_as(C.c_void_p)
    for f, reg in ((9, 0), (514, 0), (6, 0), (64, 2)):
        capfd.readouterr()
        assert alslib.cumf_weighted_rank1_loss(buf, buf, buf, buf, buf, buf, buf, buf, 1, 1, f, 0.05, reg, out, None) == 1, (f, reg)
        assert "cumf_weighted_rank1_loss" in capfd.readouterr().err
    assert alslib.cumf_weighted_rank1_loss(buf, buf, buf, buf, buf, buf, buf, buf, 1, 1, 64, 0.05, 0, None, None) == 1
    for row_w0, col_w0 in ((None, buf), (buf, None)):
        assert alslib.cumf_weighted_rank1_loss(buf, buf, buf, buf, buf, buf, row_w0, col_w0, 1, 1, 64, 0.05, 0, out, None) == 1
    for f in (9, 514, 6):
        capfd.readouterr()
        assert alslib.cumf_weighted_gram(buf, buf, 1, f, buf, None) == 1, f
        assert "cumf_weighted_gram" in capfd.readouterr().err
    assert alslib.cumf_weighted_gram(buf, None, 1, 64, buf, None) == 1  # no weights
    assert alslib.cumf_weighted_gram(None, buf, 1, 64, buf, None) == 1
    assert alslib.cumf_weighted_gram(buf, buf, 1, 64, None, None) == 1
    assert alslib.cumf_weighted_gram(buf, buf, -1, 64, buf, None) == 1


def test_python_names_and_popularity_weights(alslib):
    import inspect

    import torch

    from cumf_als_amd import als

    for name in ("weighted_gram", "update_weighted_rank1", "weighted_rank1_loss", "popularity_weights"):
        assert callable(getattr(als, name)), name
    assert inspect.signature(als.WeightedALSEngine.__init__).parameters["unobserved"].default is None
    # CSC counts 4, 1, 0, 9: the empty column gets no weight (also at exponent 0), the weights sum to c0
    counts = np.array([4, 1, 0, 9])
    r = types.SimpleNamespace(csc_indptr=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)),
                              csc_indices=torch.zeros(int(counts.sum()), dtype=torch.int32))
    for c0, e in ((1.0, 0.5), (512.0, 0.5), (3.0, 1.0), (2.0, 0.0)):
        c = als.popularity_weights(r, c0, e)
        assert c.dtype == torch.float32 and tuple(c.shape) == (4,)
        c = c.numpy().astype(np.float64)
        p = np.where(counts > 0, counts.astype(np.float64) ** e, 0.0)
        assert abs(c.sum() - c0) <= 1e-6 * c0 and c[2] == 0
        assert np.abs(c - c0 * p / p.sum()).max() <= 1e-6 * c0
    assert np.array_equal(als.popularity_weights(r, 1.0).numpy(), als.popularity_weights(r, 1.0, 0.5).numpy())
    with pytest.raises(ValueError):
        als.popularity_weights(r, -1.0)
