"""Host-side mirror of the reference's operator surface, over the C ABI of libALS.so.

* `do_als(...)` has the argument list and outputs of the reference's TensorFlow op
  `DoAls` (`tensorflow/als_tf.cc:7-30,132-136`): numpy host arrays in, (thetaT, XT,
  rmse) out.  It forwards to `cumf_doALS_ex` exactly as the TF op forwards to `doALS`.
* `Plan`, `update_fused`, `get_hermitian`, `cg_solve`, `lu_solve`, `sse` are the
  device-pointer entry points (torch CUDA tensors are used only as device memory).
* `ALSEngine` keeps one dataset resident in HBM and steps half-iterations; it is what
  bench.py times and what the multi-GPU driver (`cumf_als_amd.dist`) builds on.
* `ImplicitALSEngine` does the same for implicit feedback (include/cumf_implicit_capi.h): the
  confidence-weighted model of Hu, Koren and Volinsky, over `implicit_gram`, `update_implicit`,
  `implicit_loss`.  `get_hermitian_implicit_partial` and `implicit_finish` are the two halves of a system that several
  GPUs form together (`cumf_als_amd.dist_implicit`).
* `nnls_solve`, `update_nonneg`, `update_implicit_nonneg` (include/cumf_nnls_capi.h): non-negative least squares on
  materialised systems by block principal pivoting; both engines take `nonnegative=True` to keep every factor >= 0.
* `topk`, `ranking_metrics` (include/cumf_topk_capi.h): the k best candidates per query, scored by a fused HIP kernel
  that never writes the score matrix, and precision / recall / NDCG@k against held-out entries; both engines expose them
  as `recommend(k, side)` and `ranking_metrics(k, side)`.
* `heldout_ranks`, `rank_metrics` (include/cumf_rank_capi.h): the rank of every held-out entry among all eligible
  candidates, by the same fused scoring, and AUC / MPR / MRR / MAP / precision, recall and NDCG at any cut-off from those
  ranks; both engines expose them as `heldout_ranks(side)` and `full_ranking_metrics(side, ks)`.
* `update_biased`, `predict_biased`, `sse_biased`, `bias_mean` (include/cumf_bias_capi.h): explicit ALS with a global mean
  and user and item biases, r^ = mu + b_u + c_i + x_u . theta_i, each half-iteration the fused update at f + 2 on augmented
  tables and residual ratings; `BiasedALSEngine` trains it, and ranks and evaluates by the biased prediction.
* `update_matfree`, `matfree_available` (include/cumf_free_capi.h): the explicit half-iteration at any even 8 <= f <= 512 by a
  CG that never forms a row's system; `ALSEngine(solver="cg_matfree")` and `do_als(solver="cg_matfree")` train with it.
* `update_weighted`, `weighted_loss`, `weighted_available` (include/cumf_weighted_capi.h): the same CG with a weight on every
  stored entry and one weight w0 on everything unstored; `WeightedALSEngine` trains with it.  `weighted_gram`,
  `update_weighted_rank1`, `weighted_rank1_loss`: the same with the rank-one weight a_u c_i on the unstored entry (u, i)
  (`WeightedALSEngine(unobserved=(a, c))`; `popularity_weights` gives eALS's c).

There is no CPU path here: every call lands in a HIP kernel of libALS.so.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _libmod

SOLVER_CG, SOLVER_LU = 0, 1
CUMF_ERR_FAST_RANGE = 10001  # include/cumf_als_capi.h


def _solver_id(solver) -> int:
    if solver in (SOLVER_CG, "cg", "CG"):
        return SOLVER_CG
    if solver in (SOLVER_LU, "lu", "LU"):
        return SOLVER_LU
    raise ValueError(f"unknown solver {solver!r}")


def _hostptr(a: np.ndarray, dtype) -> C.c_void_p:
    if a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
        raise TypeError(f"expected C-contiguous {np.dtype(dtype).name} array")
    return a.ctypes.data_as(C.c_void_p)


def do_als(csrrow, csrcol, csrval, cscrow, csccol, cscval, coorow, coorowtest, coocoltest, coovaltest,
           m, n, f, nnz, nnz_test, lambda_, iters, xbatch, thetabatch, deviceid=0, *,
           thetat_init=None, xt_init=None, solver="cg", cg_iters=6, fused=True,
           exact_test_grid=False, surpass_nan=False, quiet=True, return_log=False, tt_fp16=None):
    """`DoAls` (als_tf.cc): run `iters` ALS iterations on device `deviceid`.

    Argument names follow the TF op's inputs: csrrow = CSR indptr (m+1), csrcol = CSR
    indices, cscrow = CSC row ids (nnz), csccol = CSC indptr (n+1), coorow = row of each
    CSR entry.  Returns (thetaT[n,f], XT[m,f], rmse) (+ rmse_log[iters,2] if asked).

    Initial factors default to the CLI's initialisation (main.cpp:72-78 evaluated with
    numpy's generator is NOT the same stream as libc rand(); pass `thetat_init` to
    reproduce a particular start).  tt_fp16: True / False select the fp16 Gram storage of the CG solver
    (CUMF_TT_FP16, als.cu:25-33) for this call; None (default) leaves the process-wide setting
    (`cumf_set_tt_fp16` / environment CUMF_ALS_TT_FP16) alone.  Raises RuntimeError when the opt-in gram
    mode "fast" meets data outside its range (the C entry point returns NaN and sets cumf_last_error).
    """
    lib = _libmod.load()
    if _is_matfree(solver) and not matfree_available(f):  # solver "cg_matfree": both half-iterations as update_matfree
        raise ValueError(f"solver 'cg_matfree' takes even 8 <= f <= 512 (got f = {f})")
    if thetat_init is None:
        rng = np.random.RandomState(0)
        thetat = (0.2 * rng.random_sample((n, f))).astype(np.float32)
    else:
        thetat = np.array(thetat_init, dtype=np.float32, order="C", copy=True).reshape(n, f)
    xt = (np.zeros((m, f), np.float32) if xt_init is None
          else np.array(xt_init, dtype=np.float32, order="C", copy=True).reshape(m, f))
    log = np.zeros((max(iters, 1), 2), np.float32)
    csrrow = np.ascontiguousarray(csrrow, np.int32)
    csccol = np.ascontiguousarray(csccol, np.int32)
    if len(csrrow) != m + 1 or len(csccol) != n + 1:
        raise ValueError("csrrow must hold m+1 and csccol n+1 row pointers")
    args = [
        _hostptr(csrrow, np.int32), _hostptr(np.ascontiguousarray(csrcol, np.int32), np.int32),
        _hostptr(np.ascontiguousarray(csrval, np.float32), np.float32),
        _hostptr(np.ascontiguousarray(cscrow, np.int32), np.int32), _hostptr(csccol, np.int32),
        _hostptr(np.ascontiguousarray(cscval, np.float32), np.float32),
        _hostptr(np.ascontiguousarray(coorow, np.int32), np.int32),
        _hostptr(thetat, np.float32), _hostptr(xt, np.float32),
        _hostptr(np.ascontiguousarray(coorowtest, np.int32), np.int32),
        _hostptr(np.ascontiguousarray(coocoltest, np.int32), np.int32),
        _hostptr(np.ascontiguousarray(coovaltest, np.float32), np.float32),
    ]
    prev_fp16 = lib.cumf_get_tt_fp16()  # (resolves the environment default on first use)
    if tt_fp16 is not None:
        lib.cumf_set_tt_fp16(int(bool(tt_fp16)))  # CUMF_TT_FP16 (als.cu:25-33): fp16 Gram storage for the CG solver
    try:
        lib.cumf_last_error()
        rmse = lib.cumf_doALS_ex(*args, int(m), int(n), int(f), int(nnz), int(nnz_test), float(lambda_),
                                 int(iters), int(xbatch), int(thetabatch), int(deviceid),
                                 SOLVER_CG_MATFREE if _is_matfree(solver) else _solver_id(solver), int(cg_iters),
                                 int(bool(fused)), int(bool(exact_test_grid)),
                                 int(bool(surpass_nan)), int(bool(quiet)), _hostptr(log, np.float32))
        err = lib.cumf_last_error()
    finally:
        lib.cumf_set_tt_fp16(prev_fp16)
    if err == CUMF_ERR_FAST_RANGE:
        raise RuntimeError("gram mode 'fast': a factor or a rating beyond the f16 range of the pre-split operands "
                           "(|value| >= 15.99): use the default gram mode")
    if err:
        raise RuntimeError(f"cumf_doALS_ex failed with error {err}")
    if return_log:
        return thetat, xt, float(rmse), log[:iters]
    return thetat, xt, float(rmse)


# ---------------------------------------------------------------------------------------
# device-pointer entry points (torch tensors as device memory)
# ---------------------------------------------------------------------------------------

def _dp(t, dtype=None):
    import torch

    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise TypeError("expected a contiguous CUDA tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"expected dtype {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Plan:
    """Work decomposition of one side (cumf_plan_create).  `rowptr` may be a numpy array
    or a tensor (copied to host); int32 or int64."""

    def __init__(self, rowptr, f: int, row_begin: int = 0, row_end: int | None = None, chunk: int = 0):
        lib = _libmod.load()
        if hasattr(rowptr, "detach"):
            rowptr = rowptr.detach().cpu().numpy()
        rowptr = np.ascontiguousarray(rowptr)
        if rowptr.dtype == np.int64:
            is64 = 1
        elif rowptr.dtype == np.int32:
            is64 = 0
        else:
            raise TypeError("rowptr must be int32 or int64")
        self.rows = len(rowptr) - 1
        self.row_begin = row_begin
        self.row_end = self.rows if row_end is None else row_end
        self.f = f
        self._h = C.c_void_p()
        _libmod.check(lib.cumf_plan_create(C.byref(self._h), rowptr.ctypes.data_as(C.c_void_p), is64, self.rows,
                                           self.row_begin, self.row_end, f, chunk), "cumf_plan_create")
        info = (C.c_long * 4)()
        _libmod.check(lib.cumf_plan_info(self._h, info), "cumf_plan_info")
        self.n_items, self.n_slots, self.n_multi_rows, self.chunk = (int(v) for v in info)

    @property
    def batch_rows(self) -> int:
        return self.row_end - self.row_begin

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _libmod.load().cumf_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dual_rows_probe(rowptr, f: int, chunk: int, solver="lu", materialize: bool = False, gather_rows: int = 0,
                    row_begin: int = 0, row_end: int | None = None) -> dict:
    """Host only (cumf_dual_rows_probe): the whole rows a plan of `rowptr` with this chunk counts for the dual-form LU of
    short rows -- of 1..79 ratings, of 1..95, without ratings -- and how many the route hands to it right now."""
    rowptr = np.ascontiguousarray(rowptr)
    if rowptr.dtype not in (np.int32, np.int64):
        raise TypeError("rowptr must be int32 or int64")
    rows = len(rowptr) - 1
    info = (C.c_long * 4)()
    _libmod.check(_libmod.load().cumf_dual_rows_probe(rowptr.ctypes.data_as(C.c_void_p), int(rowptr.dtype == np.int64), rows,
                                                      row_begin, rows if row_end is None else row_end, int(f), int(chunk),
                                                      _solver_id(solver), int(bool(materialize)), int(gather_rows), info),
                  "cumf_dual_rows_probe")
    return {"rows_1_79": int(info[0]), "rows_1_95": int(info[1]), "rows_empty": int(info[2]), "routed": int(info[3])}


def update_fused(plan: Plan, colidx, val, gather, update, lambda_: float, solver="cg", cg_iters: int = 6):
    """One fused half-iteration over the plan's rows (cumf_als_update_fused)."""
    import torch

    lib = _libmod.load()
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], plan.f, _solver_id(solver), 0), "cumf_check_gather_table")
    _libmod.check(lib.cumf_plan_set_gather_rows(plan._h, int(gather.shape[0])), "cumf_plan_set_gather_rows")
    _libmod.check(lib.cumf_als_update_fused(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                            _dp(gather, torch.float32), _dp(update, torch.float32), plan.f,
                                            float(lambda_), _solver_id(solver), int(cg_iters), _stream()),
                  "cumf_als_update_fused")
    return update


def matfree_available(f: int) -> bool:
    """cumf_matfree_available: the matrix-free explicit half-iteration takes even 8 <= f <= 512."""
    return bool(_libmod.load().cumf_matfree_available(int(f)))


def _is_matfree(solver) -> bool:
    # the explicit routes' own name for it: `_solver_id` keeps refusing it, as the fused and materialising entry points do
    return isinstance(solver, str) and solver == "cg_matfree"


def update_matfree(plan: Plan, colidx, val, gather, update, lambda_: float, cg_iters: int = 6):
    """One explicit half-iteration over the plan's rows that never forms a system (cumf_als_update_matfree): the CG of
    `update_fused(..., "cg")` -- warm start from `update`, at most `cg_iters` steps, exit when r.r < 1e-4 -- on
    A v = T^T (T v) + n lambda v evaluated from the stored entries; even 8 <= f <= 512.  Rows without entries get 0."""
    import torch

    if not matfree_available(plan.f):
        raise ValueError(f"update_matfree takes even 8 <= f <= 512 (got f = {plan.f})")
    if gather.dim() != 2 or update.dim() != 2 or gather.shape[1] != plan.f or update.shape[1] != plan.f:
        raise ValueError(f"update_matfree: gather and update must be [rows, {plan.f}], the plan's f "
                         f"(got {tuple(gather.shape)}, {tuple(update.shape)})")
    _libmod.check(_libmod.load().cumf_als_update_matfree(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                                         _dp(gather, torch.float32), _dp(update, torch.float32),
                                                         float(lambda_), int(cg_iters), _stream()),
                  "cumf_als_update_matfree")
    return update


SSE_BINS = 1024  # CUMF_SSE_BINS


def fused_sse_available(plan: Plan, solver="cg") -> bool:
    return bool(_libmod.load().cumf_fused_sse_available(plan._h, _solver_id(solver)))


def update_fused_sse(plan: Plan, colidx, val, gather, update, lambda_: float, solver="cg", cg_iters: int = 6, bins=None):
    """`update_fused` + the train SSE of the plan's rows for free (cumf_als_update_fused_sse): returns the fp64 bins
    tensor [SSE_BINS] it ADDED to (zeroed here when not passed in); the SSE is `bins.sum()`."""
    import torch

    lib = _libmod.load()
    if bins is None:
        bins = torch.zeros(SSE_BINS, dtype=torch.float64, device=update.device)
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], plan.f, _solver_id(solver), 0), "cumf_check_gather_table")
    _libmod.check(lib.cumf_plan_set_gather_rows(plan._h, int(gather.shape[0])), "cumf_plan_set_gather_rows")
    _libmod.check(lib.cumf_als_update_fused_sse(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                                _dp(gather, torch.float32), _dp(update, torch.float32), plan.f,
                                                float(lambda_), _solver_id(solver), int(cg_iters),
                                                _dp(bins, torch.float64), _stream()), "cumf_als_update_fused_sse")
    return bins


def quadratic_sse_terms(A, b, x, reg, out=None):
    """sum over the batch of 2 x.b - x^T A x + reg |x|^2 as a 1-element fp64 tensor (ADDED to `out` when given):
    cumf_quadratic_sse_terms -- the train SSE of materialised systems is (sum r^2 of their ratings) minus it."""
    import torch

    lib = _libmod.load()
    f = b.shape[-1]
    batch = b.numel() // f
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=b.device)
    _libmod.check(lib.cumf_quadratic_sse_terms(_dp(A, torch.float32), _dp(b, torch.float32), _dp(x, torch.float32),
                                               _dp(reg, torch.float32), batch, f, _dp(out, torch.float64), _stream()),
                  "cumf_quadratic_sse_terms")
    return out


def get_hermitian(plan: Plan, colidx, val, gather, lambda_: float, tt=None, rhs=None, want_rhs=True, half=False):
    """Materialise the Gram batch tt[rows,f,f] (+ rhs[rows,f]) of the plan's rows (cumf_get_hermitian).
    half=True (or a float16 `tt`): fp16 storage of the Gram, cumf_get_hermitian_fp16 (als.cu:335-441)."""
    import torch

    lib = _libmod.load()
    f, rows = plan.f, plan.batch_rows
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], f, SOLVER_LU, 1), "cumf_check_gather_table")
    half = half or (tt is not None and tt.dtype == torch.float16)
    if tt is None:
        tt = torch.empty((rows, f, f), dtype=torch.float16 if half else torch.float32, device=gather.device)
    if rhs is None and want_rhs:
        rhs = torch.empty((rows, f), dtype=torch.float32, device=gather.device)
    if half:
        _libmod.check(lib.cumf_get_hermitian_fp16(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                                  _dp(gather, torch.float32), _dp(tt, torch.float16),
                                                  _dp(rhs, torch.float32), f, float(lambda_), _stream()),
                      "cumf_get_hermitian_fp16")
        return tt, rhs
    _libmod.check(lib.cumf_get_hermitian(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                         _dp(gather, torch.float32), _dp(tt, torch.float32),
                                         _dp(rhs, torch.float32), f, float(lambda_), _stream()),
                  "cumf_get_hermitian")
    return tt, rhs


def get_hermitian_packed(plan: Plan, colidx, val, gather, lambda_: float, packed=None, rhs=None, want_rhs=True):
    """The Gram batch of the plan's rows as packed upper triangles packed[rows, f(f+1)/2] (+ rhs[rows,f]),
    written straight from the accumulators (cumf_get_hermitian_packed): the multi-GPU reduction payload."""
    import torch

    lib = _libmod.load()
    f, rows = plan.f, plan.batch_rows
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], f, SOLVER_LU, 1), "cumf_check_gather_table")
    if packed is None:
        packed = torch.empty((rows, f * (f + 1) // 2), dtype=torch.float32, device=gather.device)
    if rhs is None and want_rhs:
        rhs = torch.empty((rows, f), dtype=torch.float32, device=gather.device)
    _libmod.check(lib.cumf_get_hermitian_packed(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                                _dp(gather, torch.float32), _dp(packed, torch.float32),
                                                _dp(rhs, torch.float32), f, float(lambda_), _stream()),
                  "cumf_get_hermitian_packed")
    return packed, rhs


def cg_solve(A, x, b, cg_iters: int = 6):
    """Batched CG, x is the warm start and is overwritten (updateXWithCGHost, cg.h:30)."""
    import torch

    lib = _libmod.load()
    f = b.shape[-1]
    batch = b.numel() // f
    if A.dtype == torch.float16:  # updateXWithCGHost_tt_fp16 (cg.h:32)
        _libmod.check(lib.cumf_cg_solve_batched_fp16(_dp(A, torch.float16), _dp(x, torch.float32),
                                                     _dp(b, torch.float32), batch, f, int(cg_iters), _stream()),
                      "cumf_cg_solve_batched_fp16")
        return x
    _libmod.check(lib.cumf_cg_solve_batched(_dp(A, torch.float32), _dp(x, torch.float32), _dp(b, torch.float32),
                                            batch, f, int(cg_iters), _stream()), "cumf_cg_solve_batched")
    return x


def lu_solve(A, b, x=None):
    """Batched unpivoted LU solve (cublasSgetrfBatched + SgetrsBatched, als.cu:77,98)."""
    import torch

    lib = _libmod.load()
    f = b.shape[-1]
    batch = b.numel() // f
    if x is None:
        x = torch.empty_like(b)
    _libmod.check(lib.cumf_lu_solve_batched(_dp(A, torch.float32), _dp(b, torch.float32), _dp(x, torch.float32),
                                            batch, f, _stream()), "cumf_lu_solve_batched")
    return x


def pack_upper(full, packed=None):
    """full[batch, f, f] (symmetric) -> packed[batch, f(f+1)/2] upper triangles (cumf_pack_upper)."""
    import torch

    lib = _libmod.load()
    batch, f = full.shape[0], full.shape[-1]
    if packed is None:
        packed = torch.empty((batch, f * (f + 1) // 2), dtype=torch.float32, device=full.device)
    _libmod.check(lib.cumf_pack_upper(_dp(full, torch.float32), _dp(packed, torch.float32), batch, f, _stream()),
                  "cumf_pack_upper")
    return packed


def unpack_upper(packed, full):
    """packed[batch, f(f+1)/2] -> full[batch, f, f], both triangles (cumf_unpack_upper)."""
    import torch

    lib = _libmod.load()
    batch, f = full.shape[0], full.shape[-1]
    _libmod.check(lib.cumf_unpack_upper(_dp(packed, torch.float32), _dp(full, torch.float32), batch, f, _stream()),
                  "cumf_unpack_upper")
    return full


def sse(val, row, col, thetaT, XT, count: int | None = None, surpass_nan: bool = False, out=None):
    """Sum of squared errors over the first `count` ratings -> 1-element fp64 tensor (cumf_sse)."""
    import torch

    lib = _libmod.load()
    f = thetaT.shape[-1]
    if count is None:
        count = val.numel()
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=val.device)
    _libmod.check(lib.cumf_sse(_dp(val, torch.float32), _dp(row, torch.int32), _dp(col, torch.int32),
                               _dp(thetaT, torch.float32), _dp(XT, torch.float32), int(count), f,
                               int(bool(surpass_nan)), _dp(out, torch.float64), _stream()), "cumf_sse")
    return out


GRAM_AUTO, GRAM_EXACT, GRAM_FAST = 0, 1, 2


def set_gram_mode(mode) -> None:
    """Arithmetic of the Gram pass (cumf_set_gram_mode): "auto"/"split" = fp32 via exact bf16x3
    splits on the bf16 matrix pipe where available, "exact" = fp32 MFMA (fmaf-chain bits), "fast"
    (opt-in) = pre-split f16 pairs, three products, 22 significand bits, |values| < 15.99."""
    m = {"auto": GRAM_AUTO, "split": GRAM_AUTO, "exact": GRAM_EXACT, "fast": GRAM_FAST}.get(mode, mode)
    _libmod.check(_libmod.load().cumf_set_gram_mode(int(m)), "cumf_set_gram_mode")


def get_gram_mode() -> str:
    return {GRAM_EXACT: "exact", GRAM_FAST: "fast"}.get(_libmod.load().cumf_get_gram_mode(), "auto")


PRESPLIT_AUTO, PRESPLIT_OFF, PRESPLIT_ON, PRESPLIT_VERIFY = -1, 0, 1, 2


def set_presplit(mode) -> None:
    """Pre-split gather tables (cumf_set_presplit): "auto" = where the planes of the table stay in the caches (default),
    "off" / "on" = never / whenever the shape allows, "verify" = on with the last feature block unpacked (bit-identical to
    "off"; the production form multiplies that block as one packed operand: same error class, other bits)."""
    m = {"auto": PRESPLIT_AUTO, "off": PRESPLIT_OFF, "on": PRESPLIT_ON, "verify": PRESPLIT_VERIFY}.get(mode, mode)
    _libmod.check(_libmod.load().cumf_set_presplit(int(m)), "cumf_set_presplit")


def get_presplit() -> str:
    return {PRESPLIT_OFF: "off", PRESPLIT_ON: "on", PRESPLIT_VERIFY: "verify"}.get(_libmod.load().cumf_get_presplit(), "auto")


def presplit_table(table: "torch.Tensor") -> "torch.Tensor":
    """The bf16 h | m | l planes of a rows x f fp32 table as the fused calls build them (cumf_presplit_table): a uint8
    tensor [rows, cumf_presplit_pitch(f)]."""
    import torch

    lib = _libmod.load()
    rows, f = int(table.shape[0]), int(table.shape[1])
    pitch = int(lib.cumf_presplit_pitch(f))
    if pitch == 0:
        raise ValueError(f"no pre-split kernels for f = {f}")
    out = torch.empty((rows, pitch), dtype=torch.uint8, device=table.device)
    _libmod.check(lib.cumf_presplit_table(_dp(table, torch.float32), out.data_ptr(), rows, f, _stream()), "cumf_presplit_table")
    return out


def gram_fast_status() -> int:
    """Range report of gram mode "fast" since the last call (waits for the device; cumf_gram_fast_status):
    bit 0 = a factor, bit 1 = a rating beyond the f16 range; 0 = clean."""
    import ctypes as C

    flags = C.c_int(0)
    _libmod.check(_libmod.load().cumf_gram_fast_status(C.byref(flags)), "cumf_gram_fast_status")
    return int(flags.value)


def check_gram_fast() -> None:
    """In gram mode "fast": raise if a factor or a rating left the f16 range since the last check (the
    affected rows are not finite); a no-op (no device wait) in every other mode."""
    if _libmod.load().cumf_get_gram_mode() != GRAM_FAST:
        return
    flags = gram_fast_status()
    if flags:
        what = " and ".join(w for b, w in ((1, "a factor"), (2, "a rating")) if flags & b)
        raise RuntimeError(f"gram mode 'fast': {what} beyond the f16 range of the pre-split operands "
                           "(|value| >= 15.99): use the default gram mode")


def set_debug_switches(switches: int) -> None:
    """Ablation switches (1 = no solve: the Gram pass alone, ...; the results are wrong on purpose).  They
    exist only in the profiling build libALS_ablate.so (`CUMF_ALS_LIB=.../libALS_ablate.so`, used by
    tools/gram_pass_alone.py); the product library has no such entry point and this raises."""
    lib = _libmod.load()
    if not hasattr(lib, "cumf_set_debug_switches"):
        raise RuntimeError("ablation switches exist only in libALS_ablate.so (load it through CUMF_ALS_LIB)")
    _libmod.check(lib.cumf_set_debug_switches(int(switches)), "cumf_set_debug_switches")


def debug_cg_histogram(f: int):
    """Profiling build only, after running with switch 65536: rows by the number of CG iterations they ran before
    ||r||^2 < 1e-4 ended the loop (cg.cu:195); read and cleared."""
    lib = _libmod.load()
    if not hasattr(lib, "cumf_debug_cg_histogram"):
        raise RuntimeError("the CG histogram exists only in libALS_ablate.so (load it through CUMF_ALS_LIB)")
    out = (C.c_ulonglong * 16)()
    _libmod.check(lib.cumf_debug_cg_histogram(int(f), out), "cumf_debug_cg_histogram")
    return [int(v) for v in out]


def last_kernel_name() -> str:
    """Name of the Gram(+solve) kernel the last half-iteration dispatched, as rocprofv3 prints it."""
    buf = C.create_string_buffer(256)
    _libmod.check(_libmod.load().cumf_last_kernel_name(buf, 256), "cumf_last_kernel_name")
    return buf.value.decode()


def last_tile_batches():
    """(batches, rows per batch) of the pooled tile buffer in the last half-iteration (cumf_last_tile_batches): the whole rows
    of the two-wave route (LU from f = 144, materialise from f = 112) go through it in batches of at most `rows per batch`;
    (0, 0) when the call did not use the buffer.  CUMF_ALS_TILE_BUFFER_GB sizes it."""
    info = (C.c_long * 2)()
    _libmod.check(_libmod.load().cumf_last_tile_batches(info), "cumf_last_tile_batches")
    return int(info[0]), int(info[1])


def set_kernel_timing(enable: bool) -> None:
    _libmod.check(_libmod.load().cumf_set_kernel_timing(int(bool(enable))), "cumf_set_kernel_timing")


def last_kernel_ms():
    """(item_kernel_ms, reduce_kernel_ms) of the last half-iteration (HIP events on its stream)."""
    a, b = C.c_float(), C.c_float()
    _libmod.check(_libmod.load().cumf_last_kernel_ms(C.byref(a), C.byref(b)), "cumf_last_kernel_ms")
    return a.value, b.value


def kernel_ms_since_reset():
    """(item_kernel_ms, reduce_kernel_ms, launches) summed over every half-iteration launch sequence since the
    previous call (cumf_kernel_ms_since_reset): a half-iteration made of several launches is read with one call."""
    a, b, n = C.c_float(), C.c_float(), C.c_int()
    _libmod.check(_libmod.load().cumf_kernel_ms_since_reset(C.byref(a), C.byref(b), C.byref(n)),
                  "cumf_kernel_ms_since_reset")
    return a.value, b.value, n.value


def release_scratch() -> None:
    """Free the pooled scratch of the CURRENT device (tile buffers of the f >= 144 LU path, pre-split tables of gram
    mode "fast"): cumf_release_scratch.  ALSEngine.close() / DistALS.close() call it."""
    _libmod.check(_libmod.load().cumf_release_scratch(), "cumf_release_scratch")


# ---------------------------------------------------------------------------------------
# non-negative least squares and non-negative ALS (include/cumf_nnls_capi.h)
# ---------------------------------------------------------------------------------------

NNLS_MAX_F = 128


def nnls_available(f: int) -> bool:
    """Does nnls_solve take f (1 <= f <= 128)?"""
    return bool(_libmod.load().cumf_nnls_available(int(f)))


def _check_nonneg_f(f: int) -> None:
    if not (8 <= int(f) <= NNLS_MAX_F and int(f) % 2 == 0):
        raise ValueError(f"non-negative ALS takes even 8 <= f <= {NNLS_MAX_F} (got f = {f})")


def _nnls_stats(stats):
    import torch

    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < 2):
        raise TypeError("stats must be an int64 tensor of 2 entries on the device")
    return _dp(stats, torch.int64)


def nnls_solve(A, b, x, max_iters: int = 0, stats=None):
    """x = argmin_{x >= 0} 1/2 x^T A x - b^T x for each system of the batch (cumf_nnls_solve_batched): A batch x f x f
    (SPD, both triangles), b and x batch x f, fp32 on the device.  x is the warm start (passive set {x > 0}) and receives
    the solution; A and b are not modified.  max_iters: passive-set steps per system, 0 = the library default.  stats: an
    optional int64 tensor [2] that is ADDED to: (systems not converged, factorisations)."""
    import torch

    f = b.shape[-1]
    batch = b.numel() // f if f else 0
    _libmod.check(_libmod.load().cumf_nnls_solve_batched(
        _dp(A, torch.float32), _dp(b, torch.float32), _dp(x, torch.float32), batch, int(f), int(max_iters),
        _nnls_stats(stats), _stream()), "cumf_nnls_solve_batched")
    return x


def update_nonneg(plan: Plan, colidx, val, gather, update, lambda_: float, max_iters: int = 0, stats=None):
    """One explicit non-negative half-iteration over the plan's rows (cumf_als_update_nonneg): the systems of
    `get_hermitian` solved by `nnls_solve` with `update` as warm start and output; rows without ratings get 0."""
    import torch

    lib = _libmod.load()
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], plan.f, SOLVER_LU, 1), "cumf_check_gather_table")
    _libmod.check(lib.cumf_als_update_nonneg(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                             _dp(gather, torch.float32), _dp(update, torch.float32), plan.f,
                                             float(lambda_), int(max_iters), _nnls_stats(stats), _stream()),
                  "cumf_als_update_nonneg")
    return update


def update_implicit_nonneg(plan: Plan, colidx, val, gather, G, update, lambda_: float, alpha: float, reg="weighted",
                           max_iters: int = 0, stats=None):
    """One implicit non-negative half-iteration (cumf_als_update_implicit_nonneg): the systems of
    `get_hermitian_implicit` solved by `nnls_solve`; G is implicit_gram(gather); rows without entries get 0."""
    import torch

    _libmod.check(_libmod.load().cumf_als_update_implicit_nonneg(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(gather, torch.float32), _dp(G, torch.float32),
        _dp(update, torch.float32), plan.f, float(lambda_), float(alpha), _reg_id(reg), int(max_iters),
        _nnls_stats(stats), _stream()), "cumf_als_update_implicit_nonneg")
    return update


# ---------------------------------------------------------------------------------------
# top-k recommendation and ranking metrics (include/cumf_topk_capi.h)
# ---------------------------------------------------------------------------------------

def topk_available(f: int, k: int) -> bool:
    return bool(_libmod.load().cumf_topk_available(int(f), int(k)))


def _rowptr(rowptr):
    import torch

    if rowptr.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"row pointers must be int32 or int64, got {rowptr.dtype}")
    return _dp(rowptr), int(rowptr.dtype == torch.int64)


def _exclusion(exclude):
    """(rowptr, is64, colidx) arguments of an optional (rowptr, colidx) exclusion CSR; none: (None, 0, None)."""
    import torch

    if exclude is None:
        return None, 0, None
    return (*_rowptr(exclude[0]), _dp(exclude[1], torch.int32))


def topk(query, cand, k: int, exclude=None, out=None):
    """The k best candidates of every query row (cumf_topk): `query` rows x f and `cand` ncand x f fp32 on the device, the
    score of a candidate the fp32 fmaf chain of the dot product in increasing feature order.  `exclude` is an optional
    (rowptr, colidx) CSR of candidate indices per query (ascending within each row) that are never returned.  Returns
    (ids int32, scores fp32), rows x k each, best first (ties: lower index first); missing slots are -1 / -inf."""
    import torch

    rows, f = int(query.shape[0]), int(query.shape[1])
    if int(cand.shape[1]) != f:
        raise ValueError(f"query and candidate tables differ in f ({f} vs {int(cand.shape[1])})")
    if out is None:
        out = (torch.empty((rows, k), dtype=torch.int32, device=query.device),
               torch.empty((rows, k), dtype=torch.float32, device=query.device))
    ids, scores = out
    rp, rp64, ci = _exclusion(exclude)
    _libmod.check(_libmod.load().cumf_topk(
        _dp(query, torch.float32), rows, _dp(cand, torch.float32), int(cand.shape[0]), f, rp, rp64, ci, int(k),
        _dp(ids, torch.int32), _dp(scores, torch.float32), _stream()), "cumf_topk")
    return ids, scores


def ranking_metrics(ids, test_rowptr, test_colidx, test_val=None) -> dict:
    """precision@k, recall@k and NDCG@k (cumf_ranking_metrics) of `ids` (rows x k, as `topk` returns them) against a
    held-out CSR per query (column indices ascending and unique within each row); an entry is relevant when its value
    is > 0, or always without values.  Means over the queries with at least one relevant entry ("queries")."""
    import torch

    rows, k = int(ids.shape[0]), int(ids.shape[1])
    out = torch.zeros(4, dtype=torch.float64, device=ids.device)
    rp, rp64 = _rowptr(test_rowptr)
    _libmod.check(_libmod.load().cumf_ranking_metrics(
        _dp(ids, torch.int32), rows, k, rp, rp64, _dp(test_colidx, torch.int32),
        None if test_val is None else _dp(test_val, torch.float32), _dp(out, torch.float64), _stream()),
        "cumf_ranking_metrics")
    n, p, r, g = out.tolist()
    return {"queries": int(n), "precision": p, "recall": r, "ndcg": g}


def heldout_csr(row, col, val, rows: int):
    """(rowptr int64, colidx int32, val fp32) of a COO set, sorted by (row, col) with a torch sort: the held-out CSR of
    `ranking_metrics`.  Pass (col, row) for the CSC."""
    import torch

    key = (row.to(torch.int64) << 32) + col.to(torch.int64)
    order = torch.sort(key).indices
    rowptr = torch.zeros(rows + 1, dtype=torch.int64, device=row.device)
    rowptr[1:] = torch.cumsum(torch.bincount(row.to(torch.int64), minlength=rows), 0)
    return rowptr, col[order].to(torch.int32).contiguous(), val[order].to(torch.float32).contiguous()


# ---------------------------------------------------------------------------------------
# full-ranking evaluation (include/cumf_rank_capi.h)
# ---------------------------------------------------------------------------------------

def rank_available(f: int) -> bool:
    return bool(_libmod.load().cumf_rank_available(int(f)))


def heldout_ranks(query, cand, test_rowptr, test_colidx, exclude=None, out=None):
    """The rank of every held-out entry among all eligible candidates of its query (cumf_heldout_ranks): `query` rows x f
    and `cand` ncand x f fp32 on the device, scores and order as `topk`; (test_rowptr, test_colidx) the held-out CSR
    (ascending and unique within each row), `exclude` an optional (rowptr, colidx) CSR of candidates that do not count.
    Returns (ranks int32 parallel to test_colidx, n_eligible int32 per query): rank 0 is the best position, -1 marks an
    entry outside the table, excluded, or with a NaN score.  Entries outside [test_rowptr[0], test_rowptr[rows]) keep
    what `out[0]` holds (-1 without `out`)."""
    import torch

    rows, f = int(query.shape[0]), int(query.shape[1])
    if int(cand.shape[1]) != f:
        raise ValueError(f"query and candidate tables differ in f ({f} vs {int(cand.shape[1])})")
    if int(test_rowptr.shape[0]) != rows + 1:
        raise ValueError(f"test_rowptr needs rows + 1 = {rows + 1} entries, got {int(test_rowptr.shape[0])}")
    n_test = int(test_colidx.shape[0])
    if out is None:
        out = (torch.full((n_test,), -1, dtype=torch.int32, device=query.device),
               torch.empty((rows,), dtype=torch.int32, device=query.device))
    ranks, n_eligible = out
    if int(ranks.shape[0]) != n_test or int(n_eligible.shape[0]) != rows:
        raise ValueError("out must be (ranks parallel to test_colidx, n_eligible per query)")
    rp, rp64, ci = _exclusion(exclude)
    tp, tp64 = _rowptr(test_rowptr)
    _libmod.check(_libmod.load().cumf_heldout_ranks(
        _dp(query, torch.float32), rows, _dp(cand, torch.float32), int(cand.shape[0]), f, rp, rp64, ci, tp, tp64,
        _dp(test_colidx, torch.int32), n_test, _dp(ranks, torch.int32), _dp(n_eligible, torch.int32), _stream()),
        "cumf_heldout_ranks")
    return ranks, n_eligible


def rank_metrics(ranks, n_eligible, test_rowptr, test_val=None, ks=(10, 100, 1000)) -> dict:
    """AUC, MPR (expected percentile rank), MRR, MAP and precision / recall / NDCG at every cut-off of `ks`
    (cumf_rank_metrics) from what `heldout_ranks` returns; an entry is relevant when its value is > 0, or always without
    values.  "precision", "recall" and "ndcg" are dicts keyed by the cut-off."""
    import torch

    ks = [int(k) for k in ks]
    rows = int(n_eligible.shape[0])
    out = torch.zeros(6 + 3 * len(ks), dtype=torch.float64, device=ranks.device)
    rp, rp64 = _rowptr(test_rowptr)
    _libmod.check(_libmod.load().cumf_rank_metrics(
        _dp(ranks, torch.int32), _dp(n_eligible, torch.int32), rows, rp, rp64,
        None if test_val is None else _dp(test_val, torch.float32), int(ranks.shape[0]), (C.c_int * len(ks))(*ks), len(ks),
        _dp(out, torch.float64), _stream()), "cumf_rank_metrics")
    v = out.tolist()
    res = {"queries": int(v[0]), "auc_queries": int(v[1]), "auc": v[2], "mpr": v[3], "mrr": v[4], "map": v[5],
           "precision": {}, "recall": {}, "ndcg": {}}
    for c, k in enumerate(ks):
        res["precision"][k], res["recall"][k], res["ndcg"][k] = v[6 + 3 * c:9 + 3 * c]
    return res


class _Recommender:
    """recommend / ranking_metrics of a trained engine (`XT`, `thetaT`, ratings `r`), shared by both engines.  Side "x":
    the rows of XT are the queries and the rows of thetaT the candidates, the training CSR excluded; side "theta" the
    other way round, the CSC excluded."""

    def _side(self, side):
        r = self.r
        if side == "x":
            return self.XT, self.thetaT, (r.csr_indptr, r.csr_indices), (r.test_row, r.test_col, self.m)
        if side == "theta":
            return self.thetaT, self.XT, (r.csc_indptr, r.csc_indices), (r.test_col, r.test_row, self.n)
        raise ValueError(f"side must be 'x' or 'theta', got {side!r}")

    def recommend(self, k: int, side: str = "x", exclude_seen: bool = True):
        """(ids, scores) of the k best candidates of every query row of `side`, leaving out its training entries."""
        query, cand, seen, _ = self._side(side)
        return topk(query, cand, k, seen if exclude_seen else None)

    def ranking_metrics(self, k: int, side: str = "x", exclude_seen: bool = True) -> dict:
        """ranking_metrics of recommend(k, side) against the engine's test set."""
        ids, _ = self.recommend(k, side, exclude_seen)
        row, col, rows = self._side(side)[3]
        return ranking_metrics(ids, *heldout_csr(row, col, self.r.test_data, rows))

    def _heldout(self, side, exclude_seen):
        query, cand, seen, (row, col, rows) = self._side(side)
        rowptr, colidx, val = heldout_csr(row, col, self.r.test_data, rows)
        ranks, n_eligible = heldout_ranks(query, cand, rowptr, colidx, seen if exclude_seen else None)
        return ranks, n_eligible, rowptr, colidx, val

    def heldout_ranks(self, side: str = "x", exclude_seen: bool = True):
        """(ranks, n_eligible, rowptr, colidx) of the engine's test set among all candidates of `side`, its training
        entries left out: ranks is parallel to colidx, the test set as the CSR `heldout_csr` makes of it."""
        return self._heldout(side, exclude_seen)[:4]

    def full_ranking_metrics(self, side: str = "x", ks=(10, 100, 1000), exclude_seen: bool = True) -> dict:
        """rank_metrics of heldout_ranks(side) against the engine's test set."""
        ranks, n_eligible, rowptr, _, val = self._heldout(side, exclude_seen)
        return rank_metrics(ranks, n_eligible, rowptr, val, ks)


class _Engine(_Recommender):
    """What the two engines share: a dataset resident in HBM (`r`, a `cumf_als_amd.datagen.Ratings` already on the
    device), the half-iteration plans of both sides and the factors -- the reference's `thetaT` (n x f) and `XT` (m x f),
    row-contiguous f-vectors.  An engine adds `_half(plans, colidx, val, gather, update)`, one half-iteration."""

    def __init__(self, r, f: int, x_batch: int, theta_batch: int, chunk: int):
        import torch

        self.r, self.f = r, f
        self.m, self.n = r.m, r.n
        self.device = r.csr_indices.device
        self.x_plans = self._plans(r.csr_indptr, r.m, x_batch, chunk)
        self.t_plans = self._plans(r.csc_indptr, r.n, theta_batch, chunk)
        self.thetaT = torch.zeros((r.n, f), dtype=torch.float32, device=self.device)
        self.XT = torch.zeros((r.m, f), dtype=torch.float32, device=self.device)

    def _plans(self, rowptr, rows, nbatch, chunk):
        rp = rowptr.detach().cpu().numpy()
        plans = []
        for b in range(nbatch):  # als.cu:768-777
            size = rows // nbatch if b != nbatch - 1 else rows - b * (rows // nbatch)
            off = b * (rows // nbatch)
            plans.append(Plan(rp, self.f, off, off + size, chunk))
        return plans

    def init_factors(self, thetaT=None, XT=None, seed: int = 0):
        import torch

        if thetaT is None:
            g = torch.Generator(device="cpu")
            g.manual_seed(seed)
            thetaT = 0.2 * torch.rand((self.n, self.f), generator=g, dtype=torch.float32)
        self.thetaT.copy_(torch.as_tensor(thetaT).reshape(self.n, self.f))
        if XT is None:
            self.XT.zero_()
        else:
            self.XT.copy_(torch.as_tensor(XT).reshape(self.m, self.f))

    def update_x(self):
        """update X from thetaT over the CSR rows (explicit feedback: als.cu:727-855)."""
        self._half(self.x_plans, self.r.csr_indices, self.r.csr_data, self.thetaT, self.XT)

    def update_theta(self):
        """update Theta from XT over the CSC columns (explicit feedback: als.cu:857-964)."""
        self._half(self.t_plans, self.r.csc_indices, self.r.csc_data, self.XT, self.thetaT)

    def iterate(self, iters: int = 1):
        for _ in range(iters):
            self.update_x()
            self.update_theta()

    def close(self) -> None:
        """Destroy the plans and hand the library's pooled scratch of this device back (up to 48 GiB of tile buffer
        at f >= 144 that lives outside torch's caching allocator)."""
        for p in self.x_plans + self.t_plans:
            p.close()
        self.x_plans, self.t_plans = [], []
        release_scratch()


class ALSEngine(_Engine):
    """Explicit-feedback ALS on one GPU: the dataset of `_Engine` + the fused (or, above the tile kernels' range,
    materialising) half-iterations.  solver "cg_matfree" (even 8 <= f <= 512) runs every half-iteration as `update_matfree`,
    the same CG without any row's system: the route for f > 207, where "cg" and "lu" materialise f^2 floats per row; `fused`
    is unused there, `nonnegative=True` with it is refused, and `update_theta_with_train_sse` is the plain update.
    """

    def __init__(self, r, f: int, lambda_: float, solver="cg", cg_iters: int = 6, x_batch: int = 1,
                 theta_batch: int = 1, fused: bool = True, chunk: int = 0, nonnegative: bool = False):
        import torch

        self.lam = float(lambda_)
        self.solver, self.cg_iters = solver, cg_iters
        # nonnegative: every half-iteration is update_nonneg (materialise + NNLS); solver, cg_iters and fused are unused
        self.nonnegative = bool(nonnegative)
        self.matfree = _is_matfree(solver)
        if self.matfree and self.nonnegative:
            raise ValueError("solver 'cg_matfree' has no non-negative form (nonnegative=True runs update_nonneg, f <= 128)")
        if self.matfree and not matfree_available(f):
            raise ValueError(f"solver 'cg_matfree' takes even 8 <= f <= 512 (got f = {f})")
        if self.nonnegative:
            _check_nonneg_f(f)
            self.nnls_stats = torch.zeros(2, dtype=torch.int64, device=r.csr_indices.device)
        # above the tile kernels' range (f > 207) the reference's unfused data flow runs (cumf_get_hermitian + batched solver)
        self.fused = (not self.nonnegative and not self.matfree and bool(fused)
                      and bool(_libmod.load().cumf_fused_available(int(f), _solver_id(solver))))
        super().__init__(r, f, x_batch, theta_batch, chunk)
        self._tt = None
        self._rhs = None

    def _half(self, plans, colidx, val, gather, update):
        import torch

        for p in plans:
            if self.nonnegative:
                update_nonneg(p, colidx, val, gather, update, self.lam, stats=self.nnls_stats)
            elif self.matfree:
                update_matfree(p, colidx, val, gather, update, self.lam, self.cg_iters)
            elif self.fused:
                update_fused(p, colidx, val, gather, update, self.lam, self.solver, self.cg_iters)
            else:
                rows = p.batch_rows
                if self._tt is None or self._tt.shape[0] < rows:
                    self._tt = torch.empty((rows, self.f, self.f), dtype=torch.float32, device=self.device)
                    self._rhs = torch.empty((rows, self.f), dtype=torch.float32, device=self.device)
                tt, rhs = self._tt[:rows], self._rhs[:rows]
                get_hermitian(p, colidx, val, gather, self.lam, tt, rhs)
                xb = update[p.row_begin:p.row_end]
                if _solver_id(self.solver) == SOLVER_CG:
                    cg_solve(tt, xb, rhs, self.cg_iters)
                else:
                    lu_solve(tt, rhs, xb)

    def update_theta_with_train_sse(self):
        """update Theta AND return the train SSE of the new factors (fp64 scalar tensor) from the same kernels
        (cumf_als_update_fused_sse); None -- after a plain update -- when the plans cannot deliver it."""
        import torch

        if not (self.fused and all(fused_sse_available(p, self.solver) for p in self.t_plans)):
            self.update_theta()
            return None
        bins = torch.zeros(SSE_BINS, dtype=torch.float64, device=self.device)
        for p in self.t_plans:
            update_fused_sse(p, self.r.csc_indices, self.r.csc_data, self.XT, self.thetaT, self.lam, self.solver,
                             self.cg_iters, bins)
        return bins.sum()

    def rmse(self, exact_test_grid: bool = True, surpass_nan: bool = False):
        """(train, test) RMSE as als.cu:966-1020."""
        r = self.r
        tr = sse(r.csr_data, r.coo_row, r.csr_indices, self.thetaT, self.XT, r.nnz, surpass_nan)
        cnt = r.nnz_test if exact_test_grid else max(0, ((r.nnz_test - 1) // 256) * 256)
        te = sse(r.test_data, r.test_row, r.test_col, self.thetaT, self.XT, cnt, surpass_nan)
        return (float(tr.item() / max(r.nnz, 1)) ** 0.5, float(te.item() / max(r.nnz_test, 1)) ** 0.5)

    def iterate(self, iters: int = 1):
        super().iterate(iters)
        check_gram_fast()


# ---------------------------------------------------------------------------------------
# implicit feedback (include/cumf_implicit_capi.h)
# ---------------------------------------------------------------------------------------

IMPLICIT_REG_WEIGHTED, IMPLICIT_REG_PLAIN = 0, 1
SOLVER_CG_MATFREE = 2  # CUMF_SOLVER_CG_MATFREE: implicit feedback only


def _implicit_solver_id(solver) -> int:
    if solver in (SOLVER_CG_MATFREE, "cg_matfree"):
        return SOLVER_CG_MATFREE
    return _solver_id(solver)


def _reg_id(reg) -> int:
    if reg in (IMPLICIT_REG_WEIGHTED, "weighted"):
        return IMPLICIT_REG_WEIGHTED
    if reg in (IMPLICIT_REG_PLAIN, "plain"):
        return IMPLICIT_REG_PLAIN
    raise ValueError(f"unknown reg mode {reg!r} (weighted | plain)")


def implicit_available(f: int, solver="cg") -> bool:
    """cumf_implicit_available: "cg" / "lu" take even 8 <= f <= 128, "cg_matfree" even 8 <= f <= 512."""
    return bool(_libmod.load().cumf_implicit_available(int(f), _implicit_solver_id(solver)))


def implicit_gram(table, G=None):
    """G = table^T table (f x f fp32, both triangles) of a rows x f table (cumf_implicit_gram); bit-identical run to run."""
    import torch

    rows, f = int(table.shape[0]), int(table.shape[1])
    if G is None:
        G = torch.empty((f, f), dtype=torch.float32, device=table.device)
    _libmod.check(_libmod.load().cumf_implicit_gram(_dp(table, torch.float32), rows, f, _dp(G, torch.float32), _stream()),
                  "cumf_implicit_gram")
    return G


def get_hermitian_implicit(plan: Plan, colidx, val, gather, G, lambda_: float, alpha: float, reg="weighted", tt=None,
                           rhs=None):
    """The implicit systems tt[rows,f,f] = G + sum w y y^T + reg I and rhs[rows,f] = sum_{r>0} (1+w) y of the plan's rows
    (cumf_get_hermitian_implicit)."""
    import torch

    f, rows = plan.f, plan.batch_rows
    if tt is None:
        tt = torch.empty((rows, f, f), dtype=torch.float32, device=gather.device)
    if rhs is None:
        rhs = torch.empty((rows, f), dtype=torch.float32, device=gather.device)
    _libmod.check(_libmod.load().cumf_get_hermitian_implicit(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(gather, torch.float32), _dp(G, torch.float32),
        _dp(tt, torch.float32), _dp(rhs, torch.float32), f, float(lambda_), float(alpha), _reg_id(reg), _stream()),
        "cumf_get_hermitian_implicit")
    return tt, rhs


def get_hermitian_implicit_partial(plan: Plan, colidx, val, gather, lambda_: float, alpha: float, reg="weighted",
                                   packed=None, rhs=None):
    """The PARTIAL implicit systems of the plan's rows over the entries of this plan alone, as packed upper triangles
    packed[rows, f(f+1)/2] = sum w y y^T (+ lambda n_local on the diagonal when reg is "weighted") and rhs[rows,f] =
    sum_{r>0} (1+w) y (cumf_get_hermitian_implicit_partial): G is not added, so the partials of row slabs sum to the
    full system minus G -- the multi-GPU reduction payload, completed by `implicit_finish`."""
    import torch

    f, rows = plan.f, plan.batch_rows
    if packed is None:
        packed = torch.empty((rows, f * (f + 1) // 2), dtype=torch.float32, device=gather.device)
    if rhs is None:
        rhs = torch.empty((rows, f), dtype=torch.float32, device=gather.device)
    if tuple(packed.shape) != (rows, f * (f + 1) // 2) or tuple(rhs.shape) != (rows, f):
        raise ValueError(f"get_hermitian_implicit_partial: packed must be [{rows}, {f * (f + 1) // 2}] and rhs "
                         f"[{rows}, {f}] (got {tuple(packed.shape)}, {tuple(rhs.shape)})")
    _libmod.check(_libmod.load().cumf_get_hermitian_implicit_partial(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(gather, torch.float32),
        _dp(packed, torch.float32), _dp(rhs, torch.float32), f, float(lambda_), float(alpha), _reg_id(reg), _stream()),
        "cumf_get_hermitian_implicit_partial")
    return packed, rhs


def implicit_finish(packed, G, reg_add: float, tt=None):
    """tt[batch,f,f] = packed (upper triangles, mirrored) + G, then + reg_add on the diagonal (cumf_implicit_finish):
    the summed partials of `get_hermitian_implicit_partial` become solvable systems.  reg_add: lambda when reg is
    "plain", 0 when it is "weighted" (the partials carry lambda n already)."""
    import torch

    f = int(G.shape[-1])
    batch = int(packed.shape[0])
    if tuple(G.shape) != (f, f) or packed.shape[1] != f * (f + 1) // 2 or (tt is not None and tuple(tt.shape) != (batch, f, f)):
        raise ValueError(f"implicit_finish: packed [batch, f(f+1)/2], G [f, f] and tt [batch, f, f] do not agree "
                         f"({tuple(packed.shape)}, {tuple(G.shape)}, {None if tt is None else tuple(tt.shape)})")
    if tt is None:
        tt = torch.empty((batch, f, f), dtype=torch.float32, device=packed.device)
    _libmod.check(_libmod.load().cumf_implicit_finish(_dp(packed, torch.float32), _dp(G, torch.float32), float(reg_add),
                                                      _dp(tt, torch.float32), batch, f, _stream()),
                  "cumf_implicit_finish")
    return tt


def update_implicit(plan: Plan, colidx, val, gather, G, update, lambda_: float, alpha: float, reg="weighted", solver="cg",
                    cg_iters: int = 3):
    """One implicit half-iteration over the plan's rows (cumf_als_update_implicit); `update` is the CG warm start and
    receives the solution, G is implicit_gram(gather).  solver "cg", "lu" or "cg_matfree" (the operator-only CG)."""
    import torch

    _libmod.check(_libmod.load().cumf_als_update_implicit(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(gather, torch.float32), _dp(G, torch.float32),
        _dp(update, torch.float32), plan.f, float(lambda_), float(alpha), _reg_id(reg), _implicit_solver_id(solver),
        int(cg_iters),
        _stream()), "cumf_als_update_implicit")
    return update


def implicit_loss(rowptr, colidx, val, XT, thetaT, lambda_: float, alpha: float, reg="weighted", out=None):
    """The implicit objective (cumf_implicit_loss) as a 1-element fp64 tensor: rowptr/colidx/val are the CSR arrays of
    the ratings on the device (int32), XT m x f, thetaT n x f."""
    import torch

    m, f = int(XT.shape[0]), int(XT.shape[1])
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=XT.device)
    _libmod.check(_libmod.load().cumf_implicit_loss(
        _dp(rowptr, torch.int32), _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(XT, torch.float32),
        _dp(thetaT, torch.float32), m, int(thetaT.shape[0]), f, float(lambda_), float(alpha), _reg_id(reg),
        _dp(out, torch.float64), _stream()), "cumf_implicit_loss")
    return out


class ImplicitALSEngine(_Engine):
    """Implicit-feedback ALS on one GPU: the ratings of `r` (a `datagen.Ratings` on the device) are interaction
    strengths -- weight alpha |r|, preference r > 0 -- and every unstored entry counts as a preference of 0 with
    confidence 1.  Same shape as `ALSEngine`; each half-iteration forms G = Y^T Y of the fixed side once, before its
    batches.  solver "cg" (warm-started, `cg_iters` steps; rows of at most 32 entries never form their system), "lu" or
    "cg_matfree" (the same CG recurrence, no row ever forms its system); reg "weighted" (lambda n_u, the default) or
    "plain" (lambda).  "cg" and "lu" take even 8 <= f <= 128, "cg_matfree" even 8 <= f <= 512; at 128 < f <= 512
    solver "cg" runs "cg_matfree", the only CG there ("lu" and nonnegative=True stay limited to f <= 128)."""

    def __init__(self, r, f: int, lambda_: float, alpha: float, solver="cg", cg_iters: int = 3, reg="weighted",
                 x_batch: int = 1, theta_batch: int = 1, chunk: int = 0, nonnegative: bool = False):
        import torch

        # nonnegative: every half-iteration is update_implicit_nonneg (materialise + NNLS); solver and cg_iters are unused
        self.nonnegative = bool(nonnegative)
        if self.nonnegative:
            _check_nonneg_f(f)
            self.nnls_stats = torch.zeros(2, dtype=torch.int64, device=r.csr_indices.device)
        else:
            if solver in (SOLVER_CG, "cg", "CG") and 128 < f <= 512:
                solver = "cg_matfree"  # the only CG above f = 128
            if not implicit_available(f, solver):
                raise ValueError(f"implicit ALS takes even 8 <= f <= 128 with solver cg | lu and even 8 <= f <= 512 with "
                                 f"cg | cg_matfree (got f = {f}, {solver!r})")
        self.lam, self.alpha = float(lambda_), float(alpha)
        self.solver, self.cg_iters, self.reg = solver, int(cg_iters), _reg_id(reg)
        super().__init__(r, f, x_batch, theta_batch, chunk)
        self.csr_rowptr = r.csr_indptr.to(device=self.device, dtype=torch.int32).contiguous()
        self.G = torch.empty((f, f), dtype=torch.float32, device=self.device)

    def _half(self, plans, colidx, val, gather, update):
        implicit_gram(gather, self.G)
        for p in plans:
            if self.nonnegative:
                update_implicit_nonneg(p, colidx, val, gather, self.G, update, self.lam, self.alpha, self.reg,
                                       stats=self.nnls_stats)
            else:
                update_implicit(p, colidx, val, gather, self.G, update, self.lam, self.alpha, self.reg, self.solver,
                                self.cg_iters)

    def loss(self) -> float:
        """The implicit objective of the current factors (fp64)."""
        return float(implicit_loss(self.csr_rowptr, self.r.csr_indices, self.r.csr_data, self.XT, self.thetaT, self.lam,
                                   self.alpha, self.reg).item())


# ---------------------------------------------------------------------------------------
# weighted ALS (include/cumf_weighted_capi.h)
# ---------------------------------------------------------------------------------------

def weighted_available(f: int) -> bool:
    """cumf_weighted_available: weighted ALS takes even 8 <= f <= 512."""
    return bool(_libmod.load().cumf_weighted_available(int(f)))


def _check_w0(w0) -> float:
    w0 = float(w0)
    if not w0 >= 0.0:  # (NaN too)
        raise ValueError(f"w0, the weight of the unstored entries, must be >= 0 (got {w0})")
    return w0


def update_weighted(plan: Plan, colidx, val, wgt, gather, G, update, lambda_: float, w0: float = 0.0, reg="weighted",
                    cg_iters: int = 6):
    """One weighted half-iteration over the plan's rows that never forms a system (cumf_als_update_weighted): stored entry e
    has the rating val[e] and the weight wgt[e] >= 0, every unstored entry the target 0 and the weight w0 >= 0.  The CG of
    `update_matfree` -- warm start from `update`, at most `cg_iters` steps, exit when r.r < 1e-4 -- on
    A v = w0 G v + T^T ((w - w0) o (T v)) + reg v; even 8 <= f <= 512.  G is implicit_gram(gather), read only when w0 > 0
    (None is fine at w0 = 0); reg "weighted" (lambda n_u) or "plain" (lambda).  Rows without entries get 0."""
    import torch

    if not weighted_available(plan.f):
        raise ValueError(f"update_weighted takes even 8 <= f <= 512 (got f = {plan.f})")
    w0 = _check_w0(w0)
    if w0 > 0 and G is None:
        raise ValueError(f"update_weighted: w0 = {w0} > 0 needs G = implicit_gram(gather)")
    if gather.dim() != 2 or update.dim() != 2 or gather.shape[1] != plan.f or update.shape[1] != plan.f:
        raise ValueError(f"update_weighted: gather and update must be [rows, {plan.f}], the plan's f "
                         f"(got {tuple(gather.shape)}, {tuple(update.shape)})")
    if G is not None and tuple(G.shape) != (plan.f, plan.f):
        raise ValueError(f"update_weighted: G must be [{plan.f}, {plan.f}] (got {tuple(G.shape)})")
    if wgt.shape != val.shape:
        raise ValueError(f"update_weighted: wgt must be parallel to val (got {tuple(wgt.shape)}, {tuple(val.shape)})")
    _libmod.check(_libmod.load().cumf_als_update_weighted(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(wgt, torch.float32), _dp(gather, torch.float32),
        _dp(G, torch.float32), _dp(update, torch.float32), float(lambda_), w0, _reg_id(reg), int(cg_iters), _stream()),
        "cumf_als_update_weighted")
    return update


def weighted_loss(rowptr, colidx, val, wgt, XT, thetaT, lambda_: float, w0: float = 0.0, reg="weighted", out=None):
    """The weighted objective (cumf_weighted_loss) as a 1-element fp64 tensor: sum_stored w (r - x.y)^2 + w0 sum_unstored
    (x.y)^2 + the regularisers; rowptr/colidx/val/wgt are the CSR arrays on the device (rowptr int32), XT m x f,
    thetaT n x f."""
    import torch

    m, f = int(XT.shape[0]), int(XT.shape[1])
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=XT.device)
    _libmod.check(_libmod.load().cumf_weighted_loss(
        _dp(rowptr, torch.int32), _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(wgt, torch.float32),
        _dp(XT, torch.float32), _dp(thetaT, torch.float32), m, int(thetaT.shape[0]), f, float(lambda_), _check_w0(w0),
        _reg_id(reg), _dp(out, torch.float64), _stream()), "cumf_weighted_loss")
    return out


def _check_rank1_vec(name, t, rows, device=None):
    import torch

    if not hasattr(t, "is_cuda") or t.dtype != torch.float32 or t.dim() != 1 or int(t.shape[0]) != int(rows) \
            or (device is not None and t.device != device):
        raise TypeError(f"{name} must be a float32 device tensor of length {rows}")
    return t.contiguous()


def weighted_gram(table, row_w, G=None):
    """G = table^T diag(row_w) table (f x f fp32, both triangles, exactly symmetric) of a rows x f table and one weight per
    row (cumf_weighted_gram); bit-identical run to run, and with row_w = 1 the bits of `implicit_gram`."""
    import torch

    rows, f = int(table.shape[0]), int(table.shape[1])
    row_w = _check_rank1_vec("weighted_gram: row_w", row_w, rows, table.device)
    if G is None:
        G = torch.empty((f, f), dtype=torch.float32, device=table.device)
    _libmod.check(_libmod.load().cumf_weighted_gram(_dp(table, torch.float32), _dp(row_w, torch.float32), rows, f,
                                                    _dp(G, torch.float32), _stream()), "cumf_weighted_gram")
    return G


def update_weighted_rank1(plan: Plan, colidx, val, wgt, gather, G, own_w0, gather_w0, update, lambda_: float, reg="weighted",
                          cg_iters: int = 6):
    """`update_weighted` with the weight own_w0[u] * gather_w0[i] on the unstored entry (u, i) in place of one scalar
    (cumf_als_update_weighted_rank1): own_w0 has one weight per row of `update` (all of them, whatever rows the plan covers),
    gather_w0 one per row of `gather`, and G is weighted_gram(gather, gather_w0).  The same CG on
    A v = own_w0[u] G v + T^T ((w - own_w0[u] gather_w0) o (T v)) + reg v; even 8 <= f <= 512.  With gather_w0 = 1 and
    own_w0 = w0 the result is `update_weighted`'s, bit for bit.  Rows without entries get 0."""
    import torch

    if not weighted_available(plan.f):
        raise ValueError(f"update_weighted_rank1 takes even 8 <= f <= 512 (got f = {plan.f})")
    if G is None or own_w0 is None or gather_w0 is None:
        raise ValueError("update_weighted_rank1 needs G = weighted_gram(gather, gather_w0), own_w0 and gather_w0")
    if gather.dim() != 2 or update.dim() != 2 or gather.shape[1] != plan.f or update.shape[1] != plan.f:
        raise ValueError(f"update_weighted_rank1: gather and update must be [rows, {plan.f}], the plan's f "
                         f"(got {tuple(gather.shape)}, {tuple(update.shape)})")
    if tuple(G.shape) != (plan.f, plan.f):
        raise ValueError(f"update_weighted_rank1: G must be [{plan.f}, {plan.f}] (got {tuple(G.shape)})")
    if wgt.shape != val.shape:
        raise ValueError(f"update_weighted_rank1: wgt must be parallel to val (got {tuple(wgt.shape)}, {tuple(val.shape)})")
    own_w0 = _check_rank1_vec("update_weighted_rank1: own_w0", own_w0, update.shape[0], update.device)
    gather_w0 = _check_rank1_vec("update_weighted_rank1: gather_w0", gather_w0, gather.shape[0], gather.device)
    _libmod.check(_libmod.load().cumf_als_update_weighted_rank1(
        plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(wgt, torch.float32), _dp(gather, torch.float32),
        _dp(G, torch.float32), _dp(own_w0, torch.float32), _dp(gather_w0, torch.float32), _dp(update, torch.float32),
        float(lambda_), _reg_id(reg), int(cg_iters), _stream()), "cumf_als_update_weighted_rank1")
    return update


def weighted_rank1_loss(rowptr, colidx, val, wgt, XT, thetaT, row_w0, col_w0, lambda_: float, reg="weighted", out=None):
    """The objective with rank-one weights on the unstored entries (cumf_weighted_rank1_loss) as a 1-element fp64 tensor:
    sum_stored w (r - x.y)^2 + sum_unstored row_w0[u] col_w0[i] (x.y)^2 + the regularisers; rowptr/colidx/val/wgt are the CSR
    arrays on the device (rowptr int32), XT m x f, thetaT n x f, row_w0 of length m and col_w0 of length n."""
    import torch

    m, f = int(XT.shape[0]), int(XT.shape[1])
    row_w0 = _check_rank1_vec("weighted_rank1_loss: row_w0", row_w0, m, XT.device)
    col_w0 = _check_rank1_vec("weighted_rank1_loss: col_w0", col_w0, thetaT.shape[0], XT.device)
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=XT.device)
    _libmod.check(_libmod.load().cumf_weighted_rank1_loss(
        _dp(rowptr, torch.int32), _dp(colidx, torch.int32), _dp(val, torch.float32), _dp(wgt, torch.float32),
        _dp(XT, torch.float32), _dp(thetaT, torch.float32), _dp(row_w0, torch.float32), _dp(col_w0, torch.float32), m,
        int(thetaT.shape[0]), f, float(lambda_), _reg_id(reg), _dp(out, torch.float64), _stream()), "cumf_weighted_rank1_loss")
    return out


def popularity_weights(r, c0: float, exponent: float = 0.5):
    """The eALS weights of the unstored entries of each column (He et al., SIGIR 2016): c_i = c0 n_i^e / sum_j n_j^e, n_i the
    stored entries of column i of `r` (a `datagen.Ratings`; its CSC counts), as a device fp32 tensor of length r.n that sums to
    c0.  Torch only; pair it with a row vector, e.g. torch.ones(r.m), as WeightedALSEngine(unobserved=(row_w0, col_w0))."""
    import torch

    if not float(c0) >= 0.0:
        raise ValueError(f"popularity_weights: c0 must be >= 0 (got {c0})")
    counts = torch.diff(r.csc_indptr.to(torch.int64)).to(torch.float64)
    p = counts.pow(float(exponent))
    p = torch.where(counts > 0, p, torch.zeros_like(p))  # (0^0 = 1 is not a popularity)
    total = p.sum()
    if not float(total) > 0.0:
        raise ValueError("popularity_weights: the ratings have no stored entry")
    return (float(c0) * p / total).to(device=r.csc_indices.device, dtype=torch.float32)


class WeightedALSEngine(_Engine):
    """Weighted ALS on one GPU: rating r_ui of `r` (a `datagen.Ratings` on the device) counts with the weight w_ui >= 0 of
    `weights` (a device tensor parallel to r.csr_data, CSR entry order), every unstored entry is a target of 0 with the weight
    w0 >= 0.  Same shape as `ALSEngine`; every half-iteration is `update_weighted` (even 8 <= f <= 512, CG only), and with
    w0 > 0 it forms G = Y^T Y of the fixed side once, before its batches.  reg "weighted" (lambda n_u, the default) or "plain".
    w = 1, w0 = 0 is ALSEngine(solver="cg_matfree"); w = 1 + alpha |r| on ratings (r > 0) with w0 = 1 is
    ImplicitALSEngine(solver="cg_matfree").
    unobserved=(row_w0, col_w0), two fp32 device tensors of lengths m and n (finite, >= 0), weighs the unstored entry (u, i)
    by row_w0[u] col_w0[i] in place of w0 (which must then stay 0): each half forms the weighted Gram of the fixed side once
    and is `update_weighted_rank1` (on the pair scaled so that the largest gather weight is 1), and `loss()` is
    `weighted_rank1_loss`.  (full(m, w0), ones(n)) trains what w0 does, bit
    for bit; `popularity_weights` gives the eALS column weights."""

    def __init__(self, r, weights, f: int, lambda_: float, w0: float = 0.0, reg="weighted", cg_iters: int = 6,
                 x_batch: int = 1, theta_batch: int = 1, chunk: int = 0, unobserved=None):
        import torch

        if not weighted_available(f):
            raise ValueError(f"weighted ALS takes even 8 <= f <= 512 (got f = {f})")
        self.lam, self.w0 = float(lambda_), _check_w0(w0)
        self.reg, self.cg_iters = _reg_id(reg), int(cg_iters)
        dev = r.csr_indices.device
        self.row_w0 = self.col_w0 = None
        if unobserved is not None:
            if self.w0 > 0:
                raise ValueError(f"unobserved=(row_w0, col_w0) replaces w0: pass one of them (got w0 = {self.w0})")
            row_w0, col_w0 = unobserved
            self.row_w0 = _check_rank1_vec("unobserved[0] (row_w0)", row_w0, r.m, dev)
            self.col_w0 = _check_rank1_vec("unobserved[1] (col_w0)", col_w0, r.n, dev)
            for t in (self.row_w0, self.col_w0):
                if not bool((torch.isfinite(t) & (t >= 0)).all()):
                    raise ValueError("the unobserved weights must be finite and >= 0")
            # Only the products row_w0[u] col_w0[i] are the model: each half-iteration takes the pair with the largest gather
            # weight moved into the own vector (gather / max, own * max; one rounding per weight).  A constant vector on
            # either side is then the scalar route's w0 on both sides: own = w0, gather = 1 exactly, the bits of update_weighted.
            self._w0_x = self._unit_gather(self.row_w0, self.col_w0)
            self._w0_t = self._unit_gather(self.col_w0, self.row_w0)
        if not hasattr(weights, "is_cuda") or weights.device != dev or weights.dtype != torch.float32 \
                or tuple(weights.shape) != tuple(r.csr_data.shape):
            raise TypeError("weights must be a float32 tensor on the ratings' device, parallel to r.csr_data")
        if not bool((torch.isfinite(weights) & (weights >= 0)).all()):
            raise ValueError("weights must be finite and >= 0")
        super().__init__(r, f, x_batch, theta_batch, chunk)
        self.w_csr = weights.contiguous()
        # the CSC-order copy: CSR entry e = (row, col) sits at the rank of col * m + row, which a stable sort delivers; checked
        # against the dataset's own CSC arrays bit for bit, so a dataset whose two orders disagree cannot train silently
        key = r.csr_indices.to(torch.int64) * r.m + r.coo_row.to(torch.int64)
        perm = torch.sort(key, stable=True).indices
        if not (torch.equal(r.csr_data[perm].view(torch.int32), r.csc_data.view(torch.int32))
                and torch.equal(r.coo_row[perm].to(torch.int32), r.csc_indices.to(torch.int32))):
            raise ValueError("the dataset's CSC arrays are not its CSR entries sorted by (column, row): cannot place the "
                             "weights in CSC order")
        self.w_csc = self.w_csr[perm].contiguous()
        self.csr_rowptr = r.csr_indptr.to(device=self.device, dtype=torch.int32).contiguous()
        self.G = torch.empty((f, f), dtype=torch.float32, device=self.device) \
            if (self.w0 > 0 or self.row_w0 is not None) else None

    @staticmethod
    def _unit_gather(own, gather):
        top = gather.max()
        if not float(top) > 0.0:  # no weight on any unstored entry
            return own, gather
        return (own * top).contiguous(), (gather / top).contiguous()

    def _half_weighted(self, plans, colidx, val, wgt, gather, update, own_w0=None, gather_w0=None):
        if own_w0 is not None:  # rank-one weights on the unstored entries
            weighted_gram(gather, gather_w0, self.G)
            for p in plans:
                update_weighted_rank1(p, colidx, val, wgt, gather, self.G, own_w0, gather_w0, update, self.lam, self.reg,
                                      self.cg_iters)
            return
        if self.w0 > 0:
            implicit_gram(gather, self.G)
        for p in plans:
            update_weighted(p, colidx, val, wgt, gather, self.G, update, self.lam, self.w0, self.reg, self.cg_iters)

    def update_x(self):
        self._half_weighted(self.x_plans, self.r.csr_indices, self.r.csr_data, self.w_csr, self.thetaT, self.XT,
                            *(self._w0_x if self.row_w0 is not None else ()))

    def update_theta(self):
        self._half_weighted(self.t_plans, self.r.csc_indices, self.r.csc_data, self.w_csc, self.XT, self.thetaT,
                            *(self._w0_t if self.row_w0 is not None else ()))

    def loss(self) -> float:
        """The weighted objective of the current factors (fp64)."""
        if self.row_w0 is not None:
            return float(weighted_rank1_loss(self.csr_rowptr, self.r.csr_indices, self.r.csr_data, self.w_csr, self.XT,
                                             self.thetaT, self.row_w0, self.col_w0, self.lam, self.reg).item())
        return float(weighted_loss(self.csr_rowptr, self.r.csr_indices, self.r.csr_data, self.w_csr, self.XT, self.thetaT,
                                   self.lam, self.w0, self.reg).item())


# ---------------------------------------------------------------------------------------
# biased explicit ALS (include/cumf_bias_capi.h)
# ---------------------------------------------------------------------------------------

BIAS_SIDE_X, BIAS_SIDE_THETA = 0, 1


def _bias_side(side) -> int:
    if side in (BIAS_SIDE_X, "x"):
        return BIAS_SIDE_X
    if side in (BIAS_SIDE_THETA, "theta"):
        return BIAS_SIDE_THETA
    raise ValueError(f"side must be 'x' or 'theta', got {side!r}")


def bias_available(f: int, solver="cg") -> bool:
    """cumf_bias_available: even f >= 2 with a fused route at f + 2 (f <= 204 in the default gram mode)."""
    return bool(_libmod.load().cumf_bias_available(int(f), _solver_id(solver)))


def update_biased(plan: Plan, colidx, val, gather, gather_bias, update, own_bias, side, mu: float, lambda_: float,
                  lambda_bias: float, solver="cg", cg_iters: int = 6, bins=None):
    """One biased half-iteration over the plan's rows (cumf_bias_update): `plan` made at F = f + 2, `gather` and `update`
    the augmented serving tables (rows x F), `gather_bias` and `own_bias` their bias vectors, side "x" (own bias in column
    f) or "theta" (column f + 1).  With `bins` (an fp64 tensor [SSE_BINS], ADDED to) the train SSE of the plan's rows comes
    with it, where `fused_sse_available(plan, solver)`."""
    import torch

    lib = _libmod.load()
    _libmod.check(lib.cumf_check_gather_table(gather.shape[0], plan.f, _solver_id(solver), 0), "cumf_check_gather_table")
    _libmod.check(lib.cumf_plan_set_gather_rows(plan._h, int(gather.shape[0])), "cumf_plan_set_gather_rows")
    _libmod.check(lib.cumf_bias_update(plan._h, _dp(colidx, torch.int32), _dp(val, torch.float32),
                                       _dp(gather, torch.float32), _dp(gather_bias, torch.float32),
                                       _dp(update, torch.float32), _dp(own_bias, torch.float32), plan.f - 2,
                                       _bias_side(side), float(mu), float(lambda_), float(lambda_bias), _solver_id(solver),
                                       int(cg_iters), _dp(bins, torch.float64), _stream()), "cumf_bias_update")
    return update


def residual_biased(val, colidx, bias, mu: float, out=None):
    """(val - mu) - bias[colidx] in fp32, two roundings (cumf_bias_residual): the ratings a biased half-iteration solves."""
    import torch

    if out is None:
        out = torch.empty_like(val)
    _libmod.check(_libmod.load().cumf_bias_residual(_dp(val, torch.float32), _dp(colidx, torch.int32), int(val.numel()),
                                                    _dp(bias, torch.float32), float(mu), _dp(out, torch.float32), _stream()),
                  "cumf_bias_residual")
    return out


def predict_biased(rows, cols, XA, TA, mu: float, clip=None, out=None):
    """mu + the fp32 fmaf chain of XA[rows[e]] and TA[cols[e]] (cumf_bias_predict), clamped to clip = (lo, hi) when given;
    rows and cols int32 on the device."""
    import torch

    count = int(rows.numel())
    if out is None:
        out = torch.empty(count, dtype=torch.float32, device=XA.device)
    lo, hi = (float("-inf"), float("inf")) if clip is None else (float(clip[0]), float(clip[1]))
    _libmod.check(_libmod.load().cumf_bias_predict(
        _dp(rows, torch.int32), _dp(cols, torch.int32), count, _dp(XA, torch.float32), _dp(TA, torch.float32),
        int(XA.shape[1]), float(mu), lo, hi, _dp(out, torch.float32), _stream()), "cumf_bias_predict")
    return out


def sse_biased(val, row, col, XA, TA, mu: float, count: int | None = None, out=None):
    """Sum of squared errors of the biased prediction over the first `count` ratings -> 1-element fp64 tensor
    (cumf_bias_sse); bit-identical from run to run."""
    import torch

    if count is None:
        count = val.numel()
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=val.device)
    _libmod.check(_libmod.load().cumf_bias_sse(
        _dp(val, torch.float32), _dp(row, torch.int32), _dp(col, torch.int32), int(count), _dp(XA, torch.float32),
        _dp(TA, torch.float32), int(XA.shape[1]), float(mu), _dp(out, torch.float64), _stream()), "cumf_bias_sse")
    return out


def bias_mean(val, count: int | None = None, out=None):
    """The fp64 mean of the first `count` values -> 1-element fp64 tensor (cumf_bias_mean), summed in a fixed order."""
    import torch

    if count is None:
        count = val.numel()
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=val.device)
    _libmod.check(_libmod.load().cumf_bias_mean(_dp(val, torch.float32), int(count), _dp(out, torch.float64), _stream()),
                  "cumf_bias_mean")
    return out


class BiasedALSEngine(_Engine):
    """Explicit-feedback ALS with a global mean and user / item biases on one GPU: r^ = mu + b_u + c_i + x_u . theta_i,
    lambda n_u on the factors and lambda_bias n_u on the biases (lambda_bias defaults to lambda, mu to the training mean).
    `XT` (m x F) and `thetaT` (n x F), F = f + 2, are the augmented serving tables [x | b | 1] and [theta | 1 | c]: their
    plain dot product is r^ - mu, so the inherited recommend / ranking_metrics / heldout_ranks / full_ranking_metrics rank
    by the biased prediction.  `user_bias`, `item_bias` and `mu` hold the rest of the model; `factors()` the f columns."""

    def __init__(self, r, f: int, lambda_: float, lambda_bias: float | None = None, mu: float | None = None, solver="cg",
                 cg_iters: int = 6, x_batch: int = 1, theta_batch: int = 1, chunk: int = 0):
        import torch

        if not bias_available(f, solver):
            raise ValueError(f"biased ALS takes even f >= 2 with a fused half-iteration at f + 2 (f <= 204 in the default "
                             f"gram mode); got f = {f}, {solver!r}")
        self.lam = float(lambda_)
        self.lam_bias = self.lam if lambda_bias is None else float(lambda_bias)
        if not (self.lam > 0 and self.lam_bias > 0):
            raise ValueError("biased ALS needs lambda > 0 and lambda_bias > 0")
        self.solver, self.cg_iters = solver, int(cg_iters)
        super().__init__(r, f + 2, x_batch, theta_batch, chunk)  # the plans and the tables at F
        self.f, self.F = f, f + 2
        for plans, gather_rows in ((self.x_plans, r.n), (self.t_plans, r.m)):
            for p in plans:
                _libmod.check(_libmod.load().cumf_plan_set_gather_rows(p._h, int(gather_rows)), "cumf_plan_set_gather_rows")
        self.user_bias = torch.zeros(r.m, dtype=torch.float32, device=self.device)
        self.item_bias = torch.zeros(r.n, dtype=torch.float32, device=self.device)
        self.XT[:, f + 1] = 1.0
        self.thetaT[:, f] = 1.0
        if mu is None:
            mu = float(np.float32(bias_mean(r.csr_data, r.nnz).item()))
        self.mu = float(np.float32(mu))

    def factors(self):
        """(thetaT n x f, XT m x f): the factor columns of the augmented tables, as views."""
        return self.thetaT[:, :self.f], self.XT[:, :self.f]

    def init_factors(self, thetaT=None, XT=None, user_bias=None, item_bias=None, seed: int = 0):
        """thetaT n x f and XT m x f factor arrays; the default theta is the plain engine's, X and both biases 0."""
        import torch

        f = self.f
        if thetaT is None:
            g = torch.Generator(device="cpu")
            g.manual_seed(seed)
            thetaT = 0.2 * torch.rand((self.n, f), generator=g, dtype=torch.float32)
        self.thetaT[:, :f] = torch.as_tensor(thetaT).reshape(self.n, f).to(self.device)
        self.XT[:, :f] = 0.0 if XT is None else torch.as_tensor(XT).reshape(self.m, f).to(self.device)
        for own, given, rows in ((self.user_bias, user_bias, self.m), (self.item_bias, item_bias, self.n)):
            if given is None:
                own.zero_()
            else:
                own.copy_(torch.as_tensor(given).reshape(rows))
        self.XT[:, f], self.XT[:, f + 1] = self.user_bias, 1.0
        self.thetaT[:, f], self.thetaT[:, f + 1] = 1.0, self.item_bias

    def _half_x(self, bins=None):
        for p in self.x_plans:
            update_biased(p, self.r.csr_indices, self.r.csr_data, self.thetaT, self.item_bias, self.XT, self.user_bias,
                          BIAS_SIDE_X, self.mu, self.lam, self.lam_bias, self.solver, self.cg_iters, bins)

    def _half_theta(self, bins=None):
        for p in self.t_plans:
            update_biased(p, self.r.csc_indices, self.r.csc_data, self.XT, self.user_bias, self.thetaT, self.item_bias,
                          BIAS_SIDE_THETA, self.mu, self.lam, self.lam_bias, self.solver, self.cg_iters, bins)

    def update_x(self):
        """update X and the user biases from thetaT and the item biases over the CSR rows."""
        self._half_x()

    def update_theta(self):
        """update Theta and the item biases from XT and the user biases over the CSC columns."""
        self._half_theta()

    def update_theta_with_train_sse(self):
        """update_theta AND the train SSE of the new model (fp64 scalar tensor) from the same kernels; None -- after a plain
        update -- when the plans cannot deliver it (as ALSEngine.update_theta_with_train_sse)."""
        import torch

        if not all(fused_sse_available(p, self.solver) for p in self.t_plans):
            self.update_theta()
            return None
        bins = torch.zeros(SSE_BINS, dtype=torch.float64, device=self.device)
        self._half_theta(bins)
        return bins.sum()

    def train_sse(self):
        """The train SSE of the current model (fp64 scalar tensor, cumf_bias_sse)."""
        r = self.r
        return sse_biased(r.csr_data, r.coo_row, r.csr_indices, self.XT, self.thetaT, self.mu, r.nnz)[0]

    def rmse(self):
        """(train, test) RMSE of the biased prediction, unclipped."""
        r = self.r
        te = sse_biased(r.test_data, r.test_row, r.test_col, self.XT, self.thetaT, self.mu, r.nnz_test)
        return (float(self.train_sse().item() / max(r.nnz, 1)) ** 0.5, float(te.item() / max(r.nnz_test, 1)) ** 0.5)

    def predict(self, rows, cols, clip=None):
        """The predicted ratings of the pairs (rows[e], cols[e]) as an fp32 tensor on the device; clip = (lo, hi) clamps."""
        import torch

        rows = torch.as_tensor(rows).to(device=self.device, dtype=torch.int32).contiguous()
        cols = torch.as_tensor(cols).to(device=self.device, dtype=torch.int32).contiguous()
        return predict_biased(rows, cols, self.XT, self.thetaT, self.mu, clip)
