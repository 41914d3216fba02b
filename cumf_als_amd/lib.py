"""ctypes loader of `cumf_als_amd/csrc/libALS.so` (the C ABI of include/cumf_als_capi.h, cumf_dist_capi.h,
cumf_implicit_capi.h, cumf_topk_capi.h, cumf_nnls_capi.h, cumf_rank_capi.h, cumf_bias_capi.h, cumf_free_capi.h and cumf_weighted_capi.h).

The library is the product: there is no Python or CPU fallback.  `load()` raises
when the shared object is missing or lacks a declared symbol.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# CUMF_ALS_LIB: load another build of the library (kernel experiments; the profiling build libALS_ablate.so)
LIB_PATH = os.environ.get("CUMF_ALS_LIB") or os.path.join(CSRC, "libALS.so")
MAIN_PATH = os.path.join(CSRC, "main")
HUGEWIKI_PATH = os.path.join(CSRC, "hugewiki")  # the multi-GPU program (one process per GPU over RCCL)
ABLATE_LIB_PATH = os.path.join(CSRC, "libALS_ablate.so")  # -DCUMF_ABLATE=1 build (tools/gram_pass_alone.py)
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

# The C ABI, stated once: one table per header of include/, {symbol: (restype, argtypes)}.  load() applies them;
# tests/test_capi_symbols.py compares each table with its header.
_i, _l, _f = C.c_int, C.c_long, C.c_float
_vp = _ip = _fp = C.c_void_p  # any pointer | int32 array | fp32 array
_pvp = C.POINTER(C.c_void_p)
_HOST_ARGS = [_vp] * 12 + [_i, _i, _i, _l, _l, _f, _i, _i, _i, _i]  # doALS
# include/cumf_als_capi.h
C_ABI = {
    "cumf_doALS": (_f, _HOST_ARGS),
    "cumf_doALS_ex": (_f, _HOST_ARGS + [_i] * 6 + [_vp]),
    "cumf_plan_create": (_i, [_pvp, _vp, _i, _l, _l, _l, _i, _i]),
    "cumf_plan_destroy": (_i, [_vp]),
    "cumf_plan_info": (_i, [_vp, C.POINTER(_l)]),
    "cumf_dual_rows_probe": (_i, [_vp, _i, _l, _l, _l, _i, _i, _i, _i, _l, C.POINTER(_l)]),
    "cumf_plan_set_gather_rows": (_i, [_vp, _l]),
    "cumf_gram_fast_status": (_i, [C.POINTER(_i)]),
    "cumf_fused_available": (_i, [_i, _i]),
    "cumf_als_update_fused": (_i, [_vp, _ip, _fp, _fp, _fp, _i, _f, _i, _i, _vp]),
    "cumf_fused_sse_available": (_i, [_vp, _i]),
    "cumf_als_update_fused_sse": (_i, [_vp, _ip, _fp, _fp, _fp, _i, _f, _i, _i, _vp, _vp]),
    "cumf_quadratic_sse_terms": (_i, [_fp, _fp, _fp, _fp, _l, _i, _vp, _vp]),
    "cumf_get_hermitian": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _i, _f, _vp]),
    "cumf_get_hermitian_packed": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _i, _f, _vp]),
    "cumf_get_hermitian_fp16": (_i, [_vp, _ip, _fp, _fp, _vp, _fp, _i, _f, _vp]),
    "cumf_cg_solve_batched_fp16": (_i, [_vp, _fp, _fp, _l, _i, _i, _vp]),
    "cumf_set_tt_fp16": (_i, [_i]),
    "cumf_get_tt_fp16": (_i, []),
    "cumf_cg_solve_batched": (_i, [_fp, _fp, _fp, _l, _i, _i, _vp]),
    "cumf_lu_solve_batched": (_i, [_fp, _fp, _fp, _l, _i, _vp]),
    "cumf_pack_upper": (_i, [_fp, _fp, _l, _i, _vp]),
    "cumf_unpack_upper": (_i, [_fp, _fp, _l, _i, _vp]),
    "cumf_sse": (_i, [_fp, _ip, _ip, _fp, _fp, _l, _i, _i, _vp, _vp]),
    "cumf_set_gram_mode": (_i, [_i]),
    "cumf_get_gram_mode": (_i, []),
    "cumf_set_presplit": (_i, [_i]),
    "cumf_get_presplit": (_i, []),
    "cumf_presplit_pitch": (_l, [_i]),
    "cumf_presplit_table": (_i, [_vp, _vp, _l, _i, _vp]),
    "cumf_check_gather_table": (_i, [_l, _i, _i, _i]),
    "cumf_set_kernel_timing": (_i, [_i]),
    "cumf_last_kernel_ms": (_i, [C.POINTER(_f), C.POINTER(_f)]),
    "cumf_kernel_ms_since_reset": (_i, [C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "cumf_last_kernel_name": (_i, [C.c_char_p, _i]),
    "cumf_last_tile_batches": (_i, [C.POINTER(_l)]),
    "cumf_last_error": (_i, []),
    "cumf_release_scratch": (_i, []),
    "cumf_rand_init": (None, [_fp, _l, _f, _l]),
    "cumf_widen_rowptr": (_i, [_vp, _l, _l, _vp]),
    "cumf_als_version": (_i, []),
    "cumf_als_arch": (C.c_char_p, []),
}
# include/cumf_dist_capi.h (the multi-GPU half-iterations, als_dist.cpp)
DIST_ABI = {
    "cumf_comm_unique_id": (_i, [_vp]),
    "cumf_comm_create": (_i, [_pvp, _vp, _i, _i]),
    "cumf_comm_create_local": (_i, [_pvp]),
    "cumf_comm_create_custom": (_i, [_pvp, _vp, _i, _i]),
    "cumf_comm_destroy": (_i, [_vp]),
    "cumf_comm_rank": (_i, [_vp]),
    "cumf_comm_world": (_i, [_vp]),
    "cumf_comm_transport_name": (C.c_char_p, [_vp]),
    "cumf_comm_all_reduce_f64": (_i, [_vp, _vp, _l, _vp]),
    "cumf_dist_gather_create": (_i, [_pvp, _vp, _vp, _i, _i]),
    "cumf_dist_gather_update": (_i, [_vp, _vp, _ip, _fp, _fp, _fp, _f, _i, _i, _vp, _vp]),
    "cumf_dist_gather_destroy": (_i, [_vp]),
    "cumf_dist_reduce_create": (_i, [_pvp, _vp, _l, _i, _i]),
    "cumf_dist_reduce_update_theta": (_i, [_vp, _vp, _ip, _fp, _fp, _fp, _f, _i, _i, _fp, _vp, _vp]),
    "cumf_dist_reduce_destroy": (_i, [_vp]),
}
# include/cumf_implicit_capi.h (implicit feedback, als_implicit.cpp)
IMPLICIT_ABI = {
    "cumf_implicit_available": (_i, [_i, _i]),
    "cumf_implicit_gram": (_i, [_fp, _l, _i, _fp, _vp]),
    "cumf_get_hermitian_implicit": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _fp, _i, _f, _f, _i, _vp]),
    "cumf_get_hermitian_implicit_partial": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _i, _f, _f, _i, _vp]),
    "cumf_implicit_finish": (_i, [_fp, _fp, _f, _fp, _l, _i, _vp]),
    "cumf_als_update_implicit": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _i, _f, _f, _i, _i, _i, _vp]),
    "cumf_implicit_loss": (_i, [_ip, _ip, _fp, _fp, _fp, _l, _l, _i, _f, _f, _i, _vp, _vp]),
}
# include/cumf_topk_capi.h (top-k recommendation and ranking metrics, als_topk.cpp)
TOPK_ABI = {
    "cumf_topk_available": (_i, [_i, _i]),
    "cumf_topk": (_i, [_fp, _l, _fp, _l, _i, _vp, _i, _ip, _i, _ip, _fp, _vp]),
    "cumf_ranking_metrics": (_i, [_ip, _l, _i, _vp, _i, _ip, _fp, _vp, _vp]),
}
# include/cumf_nnls_capi.h (non-negative ALS, als_nnls.cpp)
NNLS_ABI = {
    "cumf_nnls_available": (_i, [_i]),
    "cumf_nnls_solve_batched": (_i, [_fp, _fp, _fp, _l, _i, _i, _vp, _vp]),
    "cumf_als_update_nonneg": (_i, [_vp, _ip, _fp, _fp, _fp, _i, _f, _i, _vp, _vp]),
    "cumf_als_update_implicit_nonneg": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _i, _f, _f, _i, _i, _vp, _vp]),
}
# include/cumf_rank_capi.h (full-ranking evaluation, als_rank.cpp)
RANK_ABI = {
    "cumf_rank_available": (_i, [_i]),
    "cumf_heldout_ranks": (_i, [_fp, _l, _fp, _l, _i, _vp, _i, _ip, _vp, _i, _ip, _l, _ip, _ip, _vp]),
    "cumf_rank_metrics": (_i, [_ip, _ip, _l, _vp, _i, _fp, _l, C.POINTER(_i), _i, _vp, _vp]),
}
# include/cumf_bias_capi.h (biased explicit ALS, als_bias.cpp)
BIAS_ABI = {
    "cumf_bias_available": (_i, [_i, _i]),
    "cumf_bias_update": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _f, _f, _i, _i, _vp, _vp]),
    "cumf_bias_residual": (_i, [_fp, _ip, _l, _fp, _f, _fp, _vp]),
    "cumf_bias_predict": (_i, [_ip, _ip, _l, _fp, _fp, _i, _f, _f, _f, _fp, _vp]),
    "cumf_bias_sse": (_i, [_fp, _ip, _ip, _l, _fp, _fp, _i, _f, _vp, _vp]),
    "cumf_bias_mean": (_i, [_fp, _l, _vp, _vp]),
}
# include/cumf_free_capi.h (the matrix-free explicit half-iteration, als_free.cpp)
FREE_ABI = {
    "cumf_matfree_available": (_i, [_i]),
    "cumf_als_update_matfree": (_i, [_vp, _ip, _fp, _fp, _fp, _f, _i, _vp]),
}
# include/cumf_weighted_capi.h (weighted ALS on the matrix-free core, als_weighted.cpp)
WEIGHTED_ABI = {
    "cumf_weighted_available": (_i, [_i]),
    "cumf_als_update_weighted": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _fp, _f, _f, _i, _i, _vp]),
    "cumf_weighted_loss": (_i, [_ip, _ip, _fp, _fp, _fp, _fp, _l, _l, _i, _f, _f, _i, _vp, _vp]),
    "cumf_weighted_gram": (_i, [_fp, _fp, _l, _i, _fp, _vp]),
    "cumf_als_update_weighted_rank1": (_i, [_vp, _ip, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _f, _i, _i, _vp]),
    "cumf_weighted_rank1_loss": (_i, [_ip, _ip, _fp, _fp, _fp, _fp, _fp, _fp, _l, _l, _i, _f, _i, _vp, _vp]),
}
ABI_BY_HEADER = {"cumf_als_capi.h": C_ABI, "cumf_dist_capi.h": DIST_ABI, "cumf_implicit_capi.h": IMPLICIT_ABI,
                 "cumf_topk_capi.h": TOPK_ABI, "cumf_nnls_capi.h": NNLS_ABI, "cumf_rank_capi.h": RANK_ABI,
                 "cumf_bias_capi.h": BIAS_ABI, "cumf_free_capi.h": FREE_ABI, "cumf_weighted_capi.h": WEIGHTED_ABI}
C_SYMBOLS, DIST_SYMBOLS, IMPLICIT_SYMBOLS = list(C_ABI), list(DIST_ABI), list(IMPLICIT_ABI)
TOPK_SYMBOLS, NNLS_SYMBOLS, RANK_SYMBOLS = list(TOPK_ABI), list(NNLS_ABI), list(RANK_ABI)
BIAS_SYMBOLS, FREE_SYMBOLS, WEIGHTED_SYMBOLS = list(BIAS_ABI), list(FREE_ABI), list(WEIGHTED_ABI)
# C++-linkage drop-in symbols (include/als.h, include/cg.h) under the reference's mangled names
CXX_SYMBOLS = [
    "_Z5doALSPKiS0_PKfS0_S0_S2_S0_PfS3_S0_S0_S2_iiillfiiii",
    "_Z17updateXWithCGHostPfS_S_iif",
    "_Z25updateXWithCGHost_tt_fp16PfS_S_iif",
    "_Z23alsUpdateFeature100HostiPKiS0_fiiPKfPfS3_i",
]

_lib = None


def build(force: bool = False) -> str:
    """Compile libALS.so and ./main for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-s", "-C", CSRC, "clean"], check=True)
    subprocess.run(["make", "-s", f"-j{os.cpu_count() or 4}", "-C", CSRC, "build"], check=True)
    return LIB_PATH


def load():
    """Load libALS.so; raise (never fall back) if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  cumf_als_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    abi = {sym: sig for table in ABI_BY_HEADER.values() for sym, sig in table.items()}
    missing = [s for s in list(abi) + CXX_SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols declared in include/: {missing}")
    if hasattr(lib, "cumf_set_debug_switches"):  # the profiling build only (libALS_ablate.so through CUMF_ALS_LIB)
        abi["cumf_set_debug_switches"] = (_i, [_i])
    for sym, (restype, argtypes) in abi.items():
        fn = getattr(lib, sym)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with HIP error {rc}")
