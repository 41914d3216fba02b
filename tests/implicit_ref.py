"""numpy reference of implicit-feedback ALS (Hu, Koren, Volinsky 2008), shared by tests/test_implicit*.py.

A stored entry (u, i, r): weight w = alpha |r|, preference p = (r > 0); unstored entries: weight 0, preference 0.
  A_u = G + sum_{i in R(u)} w y_i y_i^T + reg_u I,   b_u = sum_{i in R(u), r > 0} (1 + w) y_i,   G = Y^T Y,
reg_u = lam n_u ("weighted") or lam ("plain").
"""
import numpy as np


def reg_of(n_u, lam, reg):
    return lam * n_u if reg == "weighted" else (lam if np.isscalar(n_u) else np.full_like(n_u, lam, dtype=np.float64))


def systems(rowptr, colidx, val, Y, lam, alpha, reg="weighted", dtype=np.float64, absolute=False):
    """A (rows x f x f) and b (rows x f) of every row, evaluated in `dtype`.  absolute: the same formula on |values|
    (the scale of the rounding error of an evaluation)."""
    Y = np.asarray(Y, dtype)
    if absolute:
        Y = np.abs(Y)
    f = Y.shape[1]
    G = Y.T @ Y
    rows = len(rowptr) - 1
    A = np.empty((rows, f, f), dtype)
    b = np.zeros((rows, f), dtype)
    for u in range(rows):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        r = np.asarray(val[s:e], dtype)
        w = dtype(alpha) * np.abs(r)
        yu = Y[colidx[s:e]]
        A[u] = G + (yu * w[:, None]).T @ yu + dtype(reg_of(e - s, lam, reg)) * np.eye(f, dtype=dtype)
        c = np.where(r > 0, 1 + w, 0).astype(dtype)
        b[u] = c @ yu if e > s else 0
    return A, b


def rhs_scale(rowptr, colidx, val, Y, alpha):
    """The |b| formula (rows x f, fp64): sum (1 + w) |y| over the positive entries of every row, the scale of the rounding
    error of b."""
    rows = len(rowptr) - 1
    Ya = np.abs(np.asarray(Y, np.float64))
    cabs = np.zeros((rows, Ya.shape[1]), np.float64)
    for u in range(rows):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        c = np.where(val[s:e] > 0, 1 + alpha * np.abs(val[s:e]), 0).astype(np.float64)
        cabs[u] = c @ Ya[colidx[s:e]] if e > s else 0
    return cabs


def dense_loss(R_stored, X, Y, lam, alpha, reg="weighted"):
    """The objective by brute force over ALL entries: R_stored is an m x n array with NaN where nothing is stored."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    stored = ~np.isnan(R_stored)
    Rv = np.where(stored, R_stored, 0.0)
    c = np.where(stored, 1 + alpha * np.abs(Rv), 1.0)
    p = (stored & (Rv > 0)).astype(np.float64)
    S = X @ Y.T
    L = float((c * (p - S) ** 2).sum())
    nu, ni = stored.sum(1), stored.sum(0)
    ru = lam * nu if reg == "weighted" else np.full(len(nu), lam)
    ri = lam * ni if reg == "weighted" else np.full(len(ni), lam)
    return L + float((ru * (X ** 2).sum(1)).sum() + (ri * (Y ** 2).sum(1)).sum())


def sparse_loss(rowptr, colidx, val, X, Y, lam, alpha, reg="weighted", absolute=False):
    """<X^T X, Y^T Y>_F + sum_stored [(1 + w)(p - s)^2 - s^2] + regs, fp64 (what cumf_implicit_loss evaluates).  absolute:
    the same sum with every term replaced by its absolute value, on |X| and |Y|: <|X|^T |X|, |Y|^T |Y|>_F + sum_stored
    [(1 + w)(p + s)^2 + s^2] + regs with s = |x_u| . |y_i| (the scale of the rounding error of an evaluation, where the
    - s^2 terms may cancel the rest)."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if absolute:
        X, Y = np.abs(X), np.abs(Y)
    rowptr = np.asarray(rowptr, np.int64)
    L = float(((X.T @ X) * (Y.T @ Y)).sum())
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    col = np.asarray(colidx, np.int64)
    r = np.asarray(val, np.float64)
    s = np.einsum("ij,ij->i", X[row], Y[col])
    w = alpha * np.abs(r)
    p = (r > 0).astype(np.float64)
    L += float(((1 + w) * (p + s) ** 2 + s ** 2).sum() if absolute else ((1 + w) * (p - s) ** 2 - s ** 2).sum())
    xx, yy = (X ** 2).sum(1), (Y ** 2).sum(1)
    if reg == "weighted":
        L += lam * float(xx[row].sum() + yy[col].sum())
    else:
        L += lam * float(xx.sum() + yy.sum())
    return L
