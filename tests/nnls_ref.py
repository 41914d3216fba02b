"""fp64 numpy reference of the NNLS problem of include/cumf_nnls_capi.h, shared by tests/test_nnls*.py:

    x* = argmin_{x >= 0} 1/2 x^T A x - b^T x,   A symmetric positive definite,

the unique point with x >= 0, g = A x - b >= 0 and x_i g_i = 0.  Block principal pivoting (Kim & Park 2011) with Murty's
single-exchange backup rule, every passive-set solve by numpy in fp64.
"""
import itertools

import numpy as np


def nnls(A, b, max_steps=None):
    """(x*, passive set F as a bool array) of one SPD system, from a cold start (F empty)."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    f = b.shape[0]
    F = np.zeros(f, bool)
    best, backup = f + 1, 3
    for _ in range(max_steps or 50 * f + 50):
        x = np.zeros(f)
        if F.any():
            x[F] = np.linalg.solve(A[np.ix_(F, F)], b[F])
        y = A @ x - b
        tol = 1e-13 * f * (np.abs(b).max() + np.abs(A).max() * np.abs(x).max())
        V = (F & (x < -tol)) | (~F & (y < -tol))
        nv = int(V.sum())
        if nv == 0:
            return np.maximum(x, 0.0), F
        if nv < best:
            best, backup = nv, 3
            F ^= V
        elif backup > 0:
            backup -= 1
            F ^= V
        else:
            F[np.nonzero(V)[0].max()] ^= True
    raise RuntimeError("nnls reference did not converge")


def nnls_batch(A, b):
    """(x*, F) of every system of a batch (A: batch x f x f, b: batch x f)."""
    out = [nnls(a, v) for a, v in zip(A, b)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def brute_force(A, b):
    """The KKT point by trying all 2^f passive sets (f <= 10): the one whose solution is >= 0 with A x - b >= 0 off it."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    f = b.shape[0]
    scale = np.abs(b).max() + 1e-300
    for r in range(f + 1):
        for S in itertools.combinations(range(f), r):
            F = np.zeros(f, bool)
            F[list(S)] = True
            x = np.zeros(f)
            if r:
                x[F] = np.linalg.solve(A[np.ix_(F, F)], b[F])
            g = A @ x - b
            if (x[F] >= -1e-12 * scale).all() and (g[~F] >= -1e-12 * scale).all():
                return np.maximum(x, 0.0)
    raise RuntimeError("no KKT point found")


def masked_system(A, b, F):
    """The system of passive set F as the GPU solver forms it: the rows and columns of A outside F replaced by the
    identity, b outside F replaced by 0."""
    A = np.array(A, copy=True)
    b = np.array(b, copy=True)
    G = ~np.asarray(F, bool)
    A[G, :] = 0
    A[:, G] = 0
    A[G, G] = 1
    b[G] = 0
    return A, b


def random_spd(rng, batch, f, rank_extra=4, diag=0.1, dtype=np.float32):
    """Grams of random data plus a diagonal (SPD), stored in `dtype` exactly symmetric."""
    Z = rng.standard_normal((batch, f + rank_extra, f))
    A = np.einsum("bki,bkj->bij", Z, Z) / (f + rank_extra) + diag * np.eye(f)
    A = A.astype(dtype)
    return 0.5 * (A + np.swapaxes(A, 1, 2))  # exact in fp32: the two halves are the same value
