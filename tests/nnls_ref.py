"""fp64 numpy reference of the NNLS problem of include/cumf_nnls_capi.h, shared by tests/test_nnls*.py:

    x* = argmin_{x >= 0} 1/2 x^T A x - b^T x,   A symmetric positive definite,

the unique point with x >= 0, g = A x - b >= 0 and x_i g_i = 0.  Block principal pivoting (Kim & Park 2011) with Murty's
single-exchange backup rule, every passive-set solve by numpy in fp64.

nnls_trace records the same schedule step by step (passive sets, Murty steps, factorisations, and the margin of every sign
test), nnls_trace_fp32 emulates the GPU solver's step in fp32 numpy, and embed / load_cycling serve the systems of
tests/golden/nnls_cycling.npz, which reach the backup rule, at any f and offset (tests/test_nnls_seams_gpu.py).
"""
import collections
import itertools
import os

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


Step = collections.namedtuple("Step", "F x y V murty index margin")
Trace = collections.namedtuple("Trace", "steps converged factorisations margin x F")


def _trace(A, b, F0, max_steps, tol_f, murty):
    """The schedule of `nnls` on arrays of one dtype (A's), recorded.  V = {i in F : x_i < -tol_x} u {i in G : y_i < -tol}
    with tol = tol_f s, tol_x = tol / max_i A_ii, s = max|b| + max_i A_ii max|x_F|: tol_f = 0 tests the signs alone."""
    dt = A.dtype.type
    f = b.shape[0]
    F = np.zeros(f, bool) if F0 is None else np.array(F0, bool)
    max_d, max_b = A.diagonal().max(), np.abs(b).max()
    best, backup = f + 1, 3
    steps, n_fact, margin, converged = [], 0, np.inf, False
    for _ in range(max_steps or 50 * f + 50):
        x = np.zeros(f, dt)
        if F.any():
            x[F] = np.linalg.solve(A[np.ix_(F, F)], b[F])
            n_fact += 1
        y = np.where(F, dt(0), A @ x - b)
        s = max_b + max_d * np.abs(x).max()
        tol = dt(tol_f) * s
        tol_x = tol / max_d if max_d > 0 else dt(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = float(np.where(F, np.abs(x) * max_d, np.abs(y)).min() / s)
        margin = min(margin, m)
        V = np.where(F, x < -tol_x, y < -tol)
        nv = int(V.sum())
        flip, is_murty, index = V, False, None
        if nv and nv >= best and backup == 0 and murty:
            is_murty, index = True, int(np.nonzero(V)[0].max())
            flip = np.zeros(f, bool)
            flip[index] = True
        steps.append(Step(F.copy(), x, y, V, is_murty, index, m))
        if nv == 0:
            converged = True
            break
        if nv < best:
            best, backup = nv, 3
        elif backup > 0:
            backup -= 1
        F = F ^ flip
    last = steps[-1]
    return Trace(steps, converged, n_fact, margin, np.where(last.F, np.maximum(last.x, 0), 0).astype(dt), last.F)


def nnls_trace(A, b, F0=None, max_steps=None, murty=True):
    """The schedule of `nnls` in fp64, step by step, from the passive set F0 (cold: empty), with the signs tested against
    zero.  Trace(steps, converged, factorisations, margin, x, F):
      steps           one Step(F, x, y, V, murty, index, margin) per step: the passive set, its solution (0 off F),
                      y = A x - b off F (0 on F), the infeasible set, the exchange that follows: murty = only `index`
                      moves (Murty's backup rule), else all of V, and the step's own margin (below); the last step of a
                      converged trace has an empty V and no exchange
      converged       False when max_steps (default: nnls's) ran out; x, F are then the last iterate, clamped
      factorisations  the steps with a non-empty passive set
      margin          min over steps (Step.margin) and indices of |x_i| max_i A_ii / s on F and |y_i| / s off F, with
                      s = max|b| + max_i A_ii max|x_F|: how far every sign test of the trace is from flipping, in the
                      units of the GPU solver's tolerance f 2^-24 s
    murty=False disables the backup rule (always the full exchange): what a solver without it would do."""
    return _trace(np.asarray(A, np.float64), np.asarray(b, np.float64), F0, max_steps, 0.0, murty)


def nnls_trace_fp32(A, b, F0=None, max_steps=None):
    """The GPU solver's step emulated with numpy in fp32: A and b cast to fp32, A_FF x = b_F solved in fp32, y in fp32,
    tol = f 2^-24 s and tol_x = tol / max_i A_ii, the same schedule.  Same record as nnls_trace."""
    b = np.asarray(b, np.float32)
    return _trace(np.asarray(A, np.float32), b, F0, max_steps, b.shape[0] * 2.0 ** -24, True)


def embed(A8, b8, f, o, dtype=np.float32):
    """A small system placed at rows and columns o.. of an f x f one that takes exactly its steps: d I outside the block
    with d the block's largest diagonal entry, b = -c outside with c the block's max|b|.  Outside the block y = c > 0 at
    every step, so nothing there ever turns infeasible, and max|b| and max_i A_ii are the block's."""
    A8, b8 = np.asarray(A8), np.asarray(b8)
    n = b8.shape[0]
    assert 0 <= o and o + n <= f
    A = np.zeros((f, f), dtype)
    A[np.arange(f), np.arange(f)] = A8.diagonal().max()
    b = np.full(f, -np.abs(b8).max(), dtype)
    A[o:o + n, o:o + n] = A8
    b[o:o + n] = b8
    return A, b


def load_cycling():
    """tests/golden/nnls_cycling.npz (make_nnls_cycling.py): 8 x 8 fp32 systems whose cold-start trace takes Murty steps."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nnls_cycling.npz"))


# (f, o) at which the tests embed the cycling cases: the block below the two-word mask's split at index 64, across it
# (o = 60: indices 60..67) and above it, at both edges of several block counts NB = f / 16 + 1
CYCLING_PAIRS = [(8, 0), (15, 7), (63, 55), (64, 56), (65, 57), (72, 0), (72, 60), (100, 0), (100, 92), (127, 119),
                 (128, 60), (128, 120)]


def cycling_needs_murty():
    """Per cycling case: does a run without the backup rule (always the full exchange) tell itself apart, by not
    converging or by another factorisation count?"""
    fx = load_cycling()
    out = []
    for A, b in zip(fx["A"], fx["b"]):
        u = nnls_trace(A, b, murty=False)
        out.append(not u.converged or u.factorisations != int(nnls_trace(A, b).factorisations))
    return np.array(out)


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
