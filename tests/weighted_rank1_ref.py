"""numpy fp64 reference of weighted ALS with rank-one weights on the unstored entries (include/cumf_weighted_capi.h), shared by
tests/test_weighted_rank1*.py.

A stored entry (u, i) has the rating r and the weight w >= 0; the unstored entry (u, i) has the target 0 and the weight
a_u c_i (a >= 0 over the rows, c >= 0 over the columns):
  L = sum_stored w (r - x_u . y_i)^2 + sum_unstored a_u c_i (x_u . y_i)^2 + sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2,
  A_u = a_u G_c + sum_{i in R(u)} (w - a_u c_i) y_i y_i^T + reg_u I,   b_u = sum_{i in R(u)} w r y_i,   G_c = Y^T diag(c) Y.
One half-iteration takes `own` (indexed as the rows being updated) and `gather` (indexed as the rows of Y): on the other side
the two change places.  reg_u as in tests/weighted_ref.py.
"""
import numpy as np

from tests.weighted_ref import _coo, reg_of


def systems(rowptr, colidx, val, wgt, Y, lam, own, gather, reg="weighted", dtype=np.float64):
    """A (rows x f x f) and b (rows x f) of every row, evaluated in `dtype`; a row without entries has b = 0."""
    Y = np.asarray(Y, dtype)
    own, gather = np.asarray(own, dtype), np.asarray(gather, dtype)
    f = Y.shape[1]
    G = (Y * gather[:, None]).T @ Y
    rows = len(rowptr) - 1
    A = np.empty((rows, f, f), dtype)
    b = np.zeros((rows, f), dtype)
    for u in range(rows):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        cols = np.asarray(colidx[s:e], np.int64)
        T = Y[cols]
        w, r = np.asarray(wgt[s:e], dtype), np.asarray(val[s:e], dtype)
        A[u] = own[u] * G + (T * (w - own[u] * gather[cols])[:, None]).T @ T \
            + dtype(reg_of(e - s, lam, reg)) * np.eye(f, dtype=dtype)
        if e > s:
            b[u] = (w * r) @ T
    return A, b


def _regs(row, col, X, Y, lam, reg):
    nu, ni = np.bincount(row, minlength=len(X)), np.bincount(col, minlength=len(Y))
    return float((reg_of(nu, lam, reg) * (X ** 2).sum(1)).sum() + (reg_of(ni, lam, reg) * (Y ** 2).sum(1)).sum())


def dense_loss(rowptr, colidx, val, wgt, X, Y, lam, a, c, reg="weighted"):
    """The objective by brute force over ALL m x n entries."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    row, col = _coo(rowptr, colidx)
    W = np.outer(np.asarray(a, np.float64), np.asarray(c, np.float64))
    R = np.zeros(W.shape)
    W[row, col] = np.asarray(wgt, np.float64)
    R[row, col] = np.asarray(val, np.float64)
    return float((W * (R - X @ Y.T) ** 2).sum()) + _regs(row, col, X, Y, lam, reg)


def sparse_loss(rowptr, colidx, val, wgt, X, Y, lam, a, c, reg="weighted"):
    """sum_stored [w (r - s)^2 - a_u c_i s^2] + <X^T diag(a) X, Y^T diag(c) Y>_F + regs, fp64 (what cumf_weighted_rank1_loss
    evaluates)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    a, c = np.asarray(a, np.float64), np.asarray(c, np.float64)
    row, col = _coo(rowptr, colidx)
    r, w = np.asarray(val, np.float64), np.asarray(wgt, np.float64)
    s = np.einsum("ij,ij->i", X[row], Y[col])
    L = float((w * (r - s) ** 2 - a[row] * c[col] * s ** 2).sum())
    L += float((((X * a[:, None]).T @ X) * ((Y * c[:, None]).T @ Y)).sum())
    return L + _regs(row, col, X, Y, lam, reg)


def exact_step(rowptr, colidx, val, wgt, Y, lam, own, gather, reg="weighted"):
    """The exact minimiser of L in every x_u with Y fixed (fp64); rows without entries get 0."""
    A, b = systems(rowptr, colidx, val, wgt, Y, lam, own, gather, reg)
    X = np.zeros_like(b)
    for u in np.flatnonzero(np.diff(np.asarray(rowptr, np.int64)) > 0):
        X[u] = np.linalg.solve(A[u], b[u])
    return X
