#!/usr/bin/env python3
"""Where the weighted matrix-free CG's error against the fp64 oracle comes from, without a GPU: on the seam rows and weights of
tests/test_weighted_gpu.py, ONE CG step evaluated in fp64 except for the two sums the sparse pass accumulates in fp32, entry by
entry in entry order -- b = sum (w r) y and T^T ((w - w0) o (T x0)) -- next to the fp32 oracle.cg, which receives A and b formed
in fp64 and rounded once.  The model reproduces what the kernels measure at cg_iters = 1 (profiles/weighted/gpu_tests.txt):
the error is that accumulation over the row's entries, not the single rounding of w - w0.
  python tools/weighted_rounding_model.py [--f 8 64 256]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LAM, REG = 0.05, "plain"


def stats(v):
    return tuple(float(f"{q:.3g}") for q in (np.median(v), np.quantile(v, 0.9), v.max()))


def fp32_sums(T, coef):
    """sum_k coef[k] T[k] accumulated in fp32 in entry order, one rounding per entry (fmaf)."""
    acc = np.zeros(T.shape[1], np.float32)
    for k in range(len(coef)):
        acc = (acc.astype(np.float64) + T[k].astype(np.float64) * float(coef[k])).astype(np.float32)
    return acc.astype(np.float64)


def model_step(ref, rowptr, colidx, val, wgt, Y, x0, A64, w0):
    """x after one CG step from x0, in fp64 but for the sparse pass's two fp32 sums; rows without entries stay 0."""
    w0f = np.float32(w0)
    G64 = Y.astype(np.float64).T @ Y.astype(np.float64)
    x = np.zeros(x0.shape)
    for u in np.flatnonzero(np.diff(rowptr) > 0):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        T = Y[colidx[s:e]]
        d = (wgt[s:e] - w0f).astype(np.float32)
        c = (wgt[s:e] * val[s:e].astype(np.float32)).astype(np.float32)
        tv = (T.astype(np.float64) @ x0[u].astype(np.float64)).astype(np.float32)  # T x0, rounded once
        ax = float(w0f) * (G64 @ x0[u]) + fp32_sums(T, (tv * d).astype(np.float32)) + ref.reg_of(e - s, LAM, REG) * x0[u]
        r0 = fp32_sums(T, c) - ax
        x[u] = x0[u] + (r0 @ r0) / (r0 @ (A64[u] @ r0)) * r0
    return x


def main() -> int:
    from oracle import pyoracle as oracle
    from tests import weighted_ref as ref
    from tests.test_free_gpu import _seam_rows

    ap = argparse.ArgumentParser()
    ap.add_argument("--f", type=int, nargs="+", default=[8, 64, 256])
    a = ap.parse_args()
    oracle.build()
    lens, rowptr, colidx, val = _seam_rows()
    rng = np.random.RandomState(41)  # the weights of tests/test_weighted_gpu.py::_general
    wgt = rng.uniform(0.5, 4.0, len(val)).astype(np.float32)
    wgt[rng.random_sample(len(val)) < 0.1] = 0.0
    live = lens > 0
    for f in a.f:
        Y = (0.3 * np.random.RandomState(3).standard_normal((5000, f))).astype(np.float32)
        x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
        for w0 in (0.3, 0.0):
            A64, b64 = ref.systems(rowptr, colidx, val, wgt, Y, LAM, np.float32(w0), REG)
            x64, x32 = np.zeros(x0.shape), np.zeros(x0.shape)
            x64[live] = oracle.cg(A64[live], x0[live].astype(np.float64), b64[live], f, 1)
            x32[live] = oracle.cg(A64[live].astype(np.float32), x0[live], b64[live].astype(np.float32), f, 1)
            xm = model_step(ref, rowptr, colidx, val, wgt, Y, x0, A64, w0)
            print(f"f={f} w0={w0} {REG} iters=1, per-row max-norm distance to the fp64 oracle (median, q90, max): "
                  f"oracle32 {stats(np.abs(x32 - x64).max(1)[live])}  fp64 step on the fp32 sums "
                  f"{stats(np.abs(xm - x64).max(1)[live])}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
