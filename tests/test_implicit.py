"""Implicit-feedback ALS without a GPU: the C ABI of include/cumf_implicit_capi.h is exported and listed, and the numpy
reference that the GPU tests (tests/test_implicit_gpu.py) measure against checks itself on a tiny problem."""
import os
import re

import numpy as np
import pytest

from tests import implicit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_implicit_header_symbols_are_exported(alslib):
    from cumf_als_amd import lib

    text = open(os.path.join(ROOT, "include", "cumf_implicit_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cumf_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared and set(declared) == set(lib.IMPLICIT_SYMBOLS), (declared, lib.IMPLICIT_SYMBOLS)
    for s in declared:
        assert hasattr(alslib, s), s
    # the scope check needs no GPU
    assert alslib.cumf_implicit_available(64, 0) == 1 and alslib.cumf_implicit_available(128, 1) == 1
    assert alslib.cumf_implicit_available(8, 0) == 1
    for f in (6, 130, 200, 7):
        assert alslib.cumf_implicit_available(f, 0) == 0, f
    assert alslib.cumf_implicit_available(64, 5) == 0


def _tiny(seed=3):
    rng = np.random.RandomState(seed)
    m, n, f = 7, 9, 3
    R = np.full((m, n), np.nan)
    mask = rng.random_sample((m, n)) < 0.4
    mask[2] = False  # an empty row
    R[mask] = rng.choice([-2.0, -0.5, 0.0, 1.0, 2.5, 4.0], mask.sum())
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))])
    colidx = np.concatenate([np.nonzero(mask[u])[0] for u in range(m)])
    val = R[mask]  # row-major order = CSR order
    X = rng.standard_normal((m, f))
    Y = rng.standard_normal((n, f))
    return R, rowptr, colidx, val, X, Y


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("alpha", [1.0, 40.0])
def test_reference_systems_are_the_gradient_of_the_dense_objective(reg, alpha):
    """dL/dx_u = 2 (A_u x_u - b_u): central differences of the brute-force objective (exact for a quadratic)."""
    R, rowptr, colidx, val, X, Y = _tiny()
    lam = 0.3
    A, b = ref.systems(rowptr, colidx, val, Y, lam, alpha, reg)
    h = 1e-3
    for u in range(X.shape[0]):
        for k in range(X.shape[1]):
            Xp, Xm = X.copy(), X.copy()
            Xp[u, k] += h
            Xm[u, k] -= h
            fd = (ref.dense_loss(R, Xp, Y, lam, alpha, reg) - ref.dense_loss(R, Xm, Y, lam, alpha, reg)) / (2 * h)
            an = 2 * (A[u] @ X[u] - b[u])[k]
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (u, k, fd, an)
    assert not b[2].any()  # the empty row: b = 0, so x = 0


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_reference_sparse_loss_equals_the_dense_sum(reg):
    R, rowptr, colidx, val, X, Y = _tiny(5)
    for alpha in (1.0, 40.0):
        dense = ref.dense_loss(R, X, Y, 0.2, alpha, reg)
        sparse = ref.sparse_loss(rowptr, colidx, val, X, Y, 0.2, alpha, reg)
        assert abs(dense - sparse) <= 1e-10 * abs(dense), (dense, sparse)


@pytest.mark.parametrize("reg", ["weighted", "plain"])
def test_reference_sparse_loss_absolute_is_the_sum_of_absolute_terms(reg):
    """sparse_loss(absolute=True) against the brute-force sum over ALL entries of |x_u| . |y_i| squared plus the stored
    entries' (1 + w)(p + s)^2 + s^2 and the regularisers; it does not see the signs of the factors, bounds |L|, and the
    |b| scale of the systems is their absolute right-hand side."""
    R, rowptr, colidx, val, X, Y = _tiny(5)
    lam = 0.2
    stored = ~np.isnan(R)
    S = np.abs(X) @ np.abs(Y).T
    nu, ni = stored.sum(1), stored.sum(0)
    ru, ri = (lam * nu, lam * ni) if reg == "weighted" else (np.full(len(nu), lam), np.full(len(ni), lam))
    regs = float((ru * (X ** 2).sum(1)).sum() + (ri * (Y ** 2).sum(1)).sum())
    flip = np.random.RandomState(1).choice([-1.0, 1.0], X.shape)
    for alpha in (1.0, 40.0):
        Rv = np.where(stored, R, 0.0)
        w = np.where(stored, alpha * np.abs(Rv), 0.0)
        p = (stored & (Rv > 0)).astype(np.float64)
        want = float((S ** 2).sum() + (stored * ((1 + w) * (p + S) ** 2 + S ** 2)).sum()) + regs
        got = ref.sparse_loss(rowptr, colidx, val, X, Y, lam, alpha, reg, absolute=True)
        assert abs(got - want) <= 1e-12 * want, (got, want)
        assert got == ref.sparse_loss(rowptr, colidx, val, X * flip, -Y, lam, alpha, reg, absolute=True)
        assert abs(ref.sparse_loss(rowptr, colidx, val, X, Y, lam, alpha, reg)) <= got
        assert abs(ref.sparse_loss(rowptr, colidx, val, X * flip, -Y, lam, alpha, reg)) <= got
        _, babs = ref.systems(rowptr, colidx, val, Y, lam, alpha, reg, absolute=True)
        assert np.array_equal(ref.rhs_scale(rowptr, colidx, val, Y, alpha), babs)
