"""Inputs and references of the step-by-step tests of the explicit CG (tests/test_cg_steps.py on the CPU,
tests/test_cg_steps_gpu.py on the GPU): 41 rows of every length around the kernels' seams over a gather table of 400 rows, a
warm start large enough to keep every r.r that is compared with the exit threshold a factor of 4 away from it, three more
rows whose warm start is built to end the CG at its first step, the plain fp64 recurrence as reference and the fp32 oracle as
yardstick.  Both test files import this module, so they see the same bytes."""
import functools

import numpy as np

from tests.test_implicit_matfree_seams_gpu import CG_EXIT

N_TABLE = 400  # gather table rows
LAM = 0.05
SEED = 71
# every length 0..33 (the empty row, N = 8 / 16 / 32 of the short kernel and its `4 q < n` exits, the 32-rating stage seam),
# then rows of two chunks and last chunks of one entry at chunk = 32 and 64, and one long row
SEAM_LENS = list(range(34)) + [63, 64, 65, 96, 97, 129, 300]
# With a warm start of 0.5 N(0, 1) no row ends at its first step (the smallest r.r after step 1 is 2e-3 at f = 10 and grows
# with f), so the exit comparison would never be taken.  Three "fast" rows -- a short one, one that is whole at chunk = 64 and
# chunked at 32, one that is chunked at both -- start from their solution plus an error along ONE eigenvector of their system:
# the first step removes it and r.r drops from 9 to rounding noise (the construction of _exit_case in
# tests/test_implicit_matfree_seams_gpu.py).
FAST_LENS = [5, 40, 100]
LENS = np.array(sorted(SEAM_LENS + FAST_LENS))
ROWS = len(LENS)
FAST_ROWS = [int(np.flatnonzero(LENS == n)[-1]) for n in FAST_LENS]
assert len(SEAM_LENS) == 41 and ROWS == 44 and (np.diff(LENS) >= 0).all()  # ascending: a length range is a row range

# the f of every GPU case (tests/test_cg_steps_gpu.py), by route
F_WORKGROUP = [2, 8, 14]
F_ONE_WAVE = [16, 30, 32, 46, 48, 62, 64, 78, 80, 94, 96, 100, 110]
F_SHORT = [32, 34, 62, 64, 66, 110]
F_TWO_WAVE = [112, 126, 128, 142, 144, 158, 160, 174, 176, 190, 192, 206]
F_TWO_WAVE_CHUNKED = [112, 126, 128, 130, 142, 158, 174, 190, 206]
F_EXACT = [10, 64, 100, 128]
F_SOLVE = [2, 14, 16, 64, 126, 128, 130, 208, 256, 258, 512]
F_SOLVE_HALF = [64, 256]
F_FUSED = sorted(set(F_WORKGROUP + F_ONE_WAVE + F_SHORT + F_TWO_WAVE + F_TWO_WAVE_CHUNKED + F_EXACT))
F_TWO_STEPS_MIN = 8  # below, a few rows lie in the window around the exit threshold: one step only


def steps_for(f):
    return (1, 2) if f >= F_TWO_STEPS_MIN else (1,)


@functools.lru_cache(maxsize=1)
def rows():
    """(rowptr, colidx, val): distinct sorted columns per row, integer ratings 1..5."""
    rng = np.random.RandomState(SEED)
    rowptr = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(N_TABLE, ln, replace=False)) for ln in LENS]).astype(np.int32)
    val = rng.randint(1, 6, int(rowptr[-1])).astype(np.float32)
    for a in (rowptr, colidx, val):
        a.setflags(write=False)
    return rowptr, colidx, val


@functools.lru_cache(maxsize=None)
def table(f):
    """The gather table: 0.3 N(0, 1), mixed signs, so that the off-diagonal Gram entries cancel."""
    t = (0.3 * np.random.RandomState(SEED + 1).standard_normal((N_TABLE, f))).astype(np.float32)
    t.setflags(write=False)
    return t


def _warm_start(f, A64, b64):
    """0.5 N(0, 1); the fast rows: the solution of (A64, b64) plus an error that leaves a residual of 3 along one eigenvector
    (a middle one: neither end of the spectrum)."""
    x = (0.5 * np.random.RandomState(SEED + 2).standard_normal((ROWS, f))).astype(np.float32)
    for u in FAST_ROWS:
        lam, U = np.linalg.eigh(A64[u])
        i = f // 2
        x[u] = np.linalg.solve(A64[u], b64[u]) + 3.0 * U[:, i] / lam[i]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def warm_start(oracle, f):
    return _warm_start(f, *systems(oracle, f))


def cg_steps(A, x0, b, iters):
    """The recurrence of cg_wave_core / cumf_cg_solve_batched (the reference's cg.cu) in plain fp64: the iterate, r.r after
    the start and after every step taken, and the step at which the row ends (r.r < CG_EXIT is tested after each step, never
    at the start).  _cg_rs of tests/test_implicit_matfree_seams_gpu.py, returning x as well."""
    x = np.array(x0, np.float64)
    r = b - A @ x
    p = r.copy()
    rs = [float(r @ r)]
    for k in range(1, iters + 1):
        ap = A @ p
        a = rs[-1] / (p @ ap)
        x += a * p
        r -= a * ap
        rs.append(float(r @ r))
        if rs[-1] < CG_EXIT:
            return x, rs, k
        p = r + (rs[-1] / rs[-2]) * p
    return x, rs, iters


def reference(A64, b64, x0, iters):
    """cg_steps over a batch; a system without ratings (A = 0, b = 0) is NaN, as in the oracle and the library (0 / 0).
    Returns x64 [rows, f], r.r after step 1 (NaN for the empty systems) and the steps taken."""
    n = len(A64)
    x = np.full((n, A64.shape[-1]), np.nan)
    rs1, steps = np.full(n, np.nan), np.zeros(n, np.int64)
    for u in range(n):
        if not A64[u].any():
            continue
        x[u], rs, steps[u] = cg_steps(A64[u], x0[u], b64[u], iters)
        rs1[u] = rs[1]
    return x, rs1, steps


def exit_clear(rs1):
    """The condition of every two-step case: no row's r.r after step 1 within a factor of 4 of CG_EXIT (then fp32 ends every
    row where fp64 does).  Rows without ratings (NaN) take no part."""
    v = rs1[~np.isnan(rs1)]
    return bool(((v < CG_EXIT / 4) | (v > CG_EXIT * 4)).all())


@functools.lru_cache(maxsize=2)  # 44 f x f fp64 systems: up to 92 MB at f = 512, so only the newest are kept
def systems(oracle, f):
    """(A64, b64) of the 44 rows: oracle.gram_rhs in fp64 (NOT oracle.half_iteration(dtype=float64), which hands its result
    back rounded to fp32)."""
    rowptr, colidx, val = rows()
    A, b = oracle.gram_rhs(rowptr, colidx, val, table(f), f, LAM, dtype=np.float64)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


@functools.lru_cache(maxsize=None)
def fused_refs(oracle, f, iters):
    """(x64, x32, rs1, steps) of one fused half-iteration of `iters` CG steps over all 44 rows: the fp64 recurrence and the
    fp32 oracle (fmaf-chain Gram, then the reference's CG: it carries Gram rounding as the HIP path does)."""
    rowptr, colidx, val = rows()
    A64, b64 = systems(oracle, f)
    x0 = warm_start(oracle, f)
    x64, rs1, steps = reference(A64, b64, x0, iters)
    x32 = oracle.half_iteration(rowptr, colidx, val, table(f), x0.copy(), f, LAM, solver="cg", cg_iters=iters)
    for a in (x64, x32, rs1, steps):
        a.setflags(write=False)
    return x64, x32, rs1, steps


@functools.lru_cache(maxsize=2)
def solve_inputs(oracle, f, half=False):
    """(A, b, x0) in fp32 as als.cg_solve receives them; half: A rounded through fp16 (its storage format).  The fast rows'
    warm start is built on the very A of the case: the fp16 rounding moves the eigenvectors by far more than the step-1
    residual may hold."""
    A64, b64 = systems(oracle, f)
    A, b = A64.astype(np.float32), b64.astype(np.float32)
    if half:
        A = A.astype(np.float16).astype(np.float32)
    x0 = _warm_start(f, A.astype(np.float64), b.astype(np.float64))
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b, x0


@functools.lru_cache(maxsize=None)
def solve_refs(oracle, f, iters, half=False):
    """(x64, x32, rs1, steps) of `iters` CG steps on the materialised fp32 systems: oracle.cg in fp64 on the very values the
    kernel reads (its agreement with cg_steps is a CPU test) and oracle.cg in fp32."""
    A, b, x0 = solve_inputs(oracle, f, half)
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    _, rs1, steps = reference(A64, b64, x0, iters)
    x64 = oracle.cg(A64, x0.astype(np.float64), b64, f, iters)
    x32 = oracle.cg(A, x0, b, f, iters)
    for a in (x64, x32, rs1, steps):
        a.setflags(write=False)
    return x64, x32, rs1, steps


def train_sse(x, f, row_begin=0, row_end=ROWS):
    """fp64 sum of (r - x_u . t_v)^2 over the ratings of the rows [row_begin, row_end) that have any, on the factors x."""
    rowptr, colidx, val = rows()
    T = table(f).astype(np.float64)
    sse = 0.0
    for u in range(row_begin, row_end):
        s, e = rowptr[u], rowptr[u + 1]
        if e > s:
            sse += float(((val[s:e].astype(np.float64) - T[colidx[s:e]] @ x[u].astype(np.float64)) ** 2).sum())
    return sse
