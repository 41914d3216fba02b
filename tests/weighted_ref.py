"""numpy fp64 reference of weighted ALS (include/cumf_weighted_capi.h), shared by tests/test_weighted*.py.

A stored entry (u, i) has the rating r and the weight w >= 0; every unstored entry has the target 0 and the weight w0 >= 0:
  L = sum_stored w (r - x_u . y_i)^2 + w0 sum_unstored (x_u . y_i)^2 + sum_u reg_u |x_u|^2 + sum_i reg_i |y_i|^2,
  A_u = w0 G + sum_{i in R(u)} (w - w0) y_i y_i^T + reg_u I,   b_u = sum_{i in R(u)} w r y_i,   G = Y^T Y.
reg_u is what the kernels evaluate in fp32: (float)n_u * lam ("weighted"; n_u counts the stored entries, those of weight 0
included) or lam ("plain").
"""
import numpy as np


def reg_of(n, lam, reg="weighted"):
    """The fp32 value the kernels add to the diagonal, as a Python float; n a count or an array of counts."""
    lam32 = np.float32(lam)
    if reg == "weighted":
        return (np.asarray(n).astype(np.float32) * lam32).astype(np.float64) if np.ndim(n) else float(np.float32(n) * lam32)
    if reg != "plain":
        raise ValueError(reg)
    return np.full(np.shape(n), float(lam32)) if np.ndim(n) else float(lam32)


def systems(rowptr, colidx, val, wgt, Y, lam, w0, reg="weighted", dtype=np.float64):
    """A (rows x f x f) and b (rows x f) of every row, evaluated in `dtype`; a row without entries has b = 0 (and
    A = w0 G + reg I)."""
    Y = np.asarray(Y, dtype)
    f = Y.shape[1]
    G = Y.T @ Y
    rows = len(rowptr) - 1
    A = np.empty((rows, f, f), dtype)
    b = np.zeros((rows, f), dtype)
    for u in range(rows):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        T = Y[colidx[s:e]]
        w, r = np.asarray(wgt[s:e], dtype), np.asarray(val[s:e], dtype)
        A[u] = dtype(w0) * G + (T * (w - dtype(w0))[:, None]).T @ T + dtype(reg_of(e - s, lam, reg)) * np.eye(f, dtype=dtype)
        if e > s:
            b[u] = (w * r) @ T
    return A, b


def _coo(rowptr, colidx):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), np.asarray(colidx, np.int64)


def dense_loss(rowptr, colidx, val, wgt, X, Y, lam, w0, reg="weighted"):
    """The objective by brute force over ALL m x n entries."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    m, n = len(X), len(Y)
    row, col = _coo(rowptr, colidx)
    W = np.full((m, n), float(w0))
    R = np.zeros((m, n))
    W[row, col] = np.asarray(wgt, np.float64)
    R[row, col] = np.asarray(val, np.float64)
    L = float((W * (R - X @ Y.T) ** 2).sum())
    nu, ni = np.bincount(row, minlength=m), np.bincount(col, minlength=n)
    return L + float((reg_of(nu, lam, reg) * (X ** 2).sum(1)).sum() + (reg_of(ni, lam, reg) * (Y ** 2).sum(1)).sum())


def sparse_loss(rowptr, colidx, val, wgt, X, Y, lam, w0, reg="weighted"):
    """w0 (<X^T X, Y^T Y>_F - sum_stored s^2) + sum_stored w (r - s)^2 + regs, fp64 (what cumf_weighted_loss evaluates)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    row, col = _coo(rowptr, colidx)
    r, w = np.asarray(val, np.float64), np.asarray(wgt, np.float64)
    s = np.einsum("ij,ij->i", X[row], Y[col])
    L = float(w0) * (float(((X.T @ X) * (Y.T @ Y)).sum()) - float((s ** 2).sum())) + float((w * (r - s) ** 2).sum())
    nu, ni = np.bincount(row, minlength=len(X)), np.bincount(col, minlength=len(Y))
    return L + float((reg_of(nu, lam, reg) * (X ** 2).sum(1)).sum() + (reg_of(ni, lam, reg) * (Y ** 2).sum(1)).sum())


def exact_step(rowptr, colidx, val, wgt, Y, lam, w0, reg="weighted"):
    """The exact minimiser of L in every x_u with Y fixed (fp64); rows without entries get 0."""
    A, b = systems(rowptr, colidx, val, wgt, Y, lam, w0, reg)
    X = np.zeros_like(b)
    for u in np.flatnonzero(np.diff(np.asarray(rowptr, np.int64)) > 0):
        X[u] = np.linalg.solve(A[u], b[u])
    return X


def transpose(rowptr, colidx, val, wgt, n):
    """The CSC arrays (as the CSR of the transpose) of an m x n CSR with column-sorted rows: colptr, row ids, val, wgt."""
    row, col = _coo(rowptr, colidx)
    order = np.lexsort((row, col))
    colptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]).astype(np.int32)
    return colptr, row[order].astype(np.int32), np.asarray(val)[order], np.asarray(wgt)[order]
