"""numpy reference of the matrix-free explicit half-iteration (include/cumf_free_capi.h), shared by tests/test_free*.py.

A row u with n stored entries (i, r): T = the n x f block of gathered rows y_i,
  A_u = T^T T + reg I,  reg = (float)n * lam evaluated in fp32 (oracle/als_oracle_impl.h),  b_u = T^T r.
"""
import numpy as np

CG_EXIT = 1e-4  # the r.r below which a row's CG ends (CG_ERROR of the reference's cg.cu)


def reg_of(n, lam):
    return float(np.float32(n) * np.float32(lam))


def systems(rowptr, colidx, val, Y, lam, dtype=np.float64):
    """A (rows x f x f) and b (rows x f) of every row, evaluated in `dtype`; a row without entries has A = 0, b = 0."""
    Y = np.asarray(Y, dtype)
    f = Y.shape[1]
    rows = len(rowptr) - 1
    A = np.zeros((rows, f, f), dtype)
    b = np.zeros((rows, f), dtype)
    for u in range(rows):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        if e == s:
            continue
        T = Y[colidx[s:e]]
        A[u] = T.T @ T + dtype(reg_of(e - s, lam)) * np.eye(f, dtype=dtype)
        b[u] = np.asarray(val[s:e], dtype) @ T
    return A, b


def matfree_cg_uniform(cols, vals, Y, x0, lam, cg_iters):
    """`matfree_cg` for rows of one common length n > 0, all rows at once: cols, vals are rows x n."""
    T = np.asarray(Y, np.float64)[cols]  # rows x n x f
    vals = np.asarray(vals, np.float64)
    reg = reg_of(cols.shape[1], lam)
    op = lambda v: np.einsum("rnf,rn->rf", T, np.einsum("rnf,rf->rn", T, v)) + reg * v  # noqa: E731
    dot = lambda u, v: np.einsum("rf,rf->r", u, v)  # noqa: E731
    x = np.array(x0, np.float64)
    r = np.einsum("rnf,rn->rf", T, vals) - op(x)
    p = r.copy()
    rsold = dot(r, r)
    live = np.ones(len(x), bool)
    for _ in range(cg_iters):
        ap = op(p)
        a = np.where(live, rsold / np.where(live, dot(p, ap), 1.0), 0.0)  # an ended row is frozen
        x += a[:, None] * p
        r -= a[:, None] * ap
        rsnew = dot(r, r)
        live &= rsnew >= CG_EXIT
        p = np.where(live[:, None], r + (rsnew / np.where(live, rsold, 1.0))[:, None] * p, p)
        rsold = np.where(live, rsnew, rsold)
    return x


def matfree_cg(rowptr, colidx, val, Y, x0, lam, cg_iters):
    """The operator-only CG in fp64: A_u p = T^T (T p) + reg p from the stored entries, never forming A_u.  The recurrence of
    oracle.cg (warm start x0, at most cg_iters steps, exit when r.r < 1e-4 after a step), checked per row; rows without
    entries get 0.  Returns x and the step at which each row ended."""
    Y = np.asarray(Y, np.float64)
    x = np.array(x0, np.float64)
    steps = np.zeros(len(rowptr) - 1, np.int64)
    for u in range(len(rowptr) - 1):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        if e == s:
            x[u] = 0
            continue
        T = Y[colidx[s:e]]
        reg = reg_of(e - s, lam)
        op = lambda v: T.T @ (T @ v) + reg * v  # noqa: E731
        xu = x[u].copy()
        r = np.asarray(val[s:e], np.float64) @ T - op(xu)
        p = r.copy()
        rsold = r @ r
        for k in range(1, cg_iters + 1):
            ap = op(p)
            a = rsold / (p @ ap)
            xu += a * p
            r -= a * ap
            rsnew = r @ r
            steps[u] = k
            if rsnew < CG_EXIT:
                break
            p = r + (rsnew / rsold) * p
            rsold = rsnew
        x[u] = xu
    return x, steps
