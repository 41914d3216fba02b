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
