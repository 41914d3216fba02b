#!/usr/bin/env python3
"""Times the non-negative explicit block solver (ALSEngine(solver="block_nonneg")) at the Netflix shape against the
unconstrained block solver of the same build, and at f <= 128 against nonnegative=True (materialise + NNLS), by
tools/block_time.py's protocol: one process, device events around each half-iteration, configurations alternated iteration by
iteration, median of --iters after --warmup.  One JSON line per f.  --converge F ...: at each F, --conv-iters iterations of
every configuration (one sweep) from the same start: train / test RMSE after the last, and for block_nonneg the eliminations
per block step (nnls_stats[1] over rows with entries x blocks x sweeps) of each iteration.
  python tools/block_nonneg_time.py [--f 64 128 256 512] [--iters 3] [--warmup 1] [--converge 64 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cumf_als_amd import als, datagen  # noqa: E402
from tools.block_time import alternated  # noqa: E402
from tools.free_time import timed_iteration  # noqa: E402

NNLS_MAX_F = 128  # nonnegative=True ends there


def engine(r, f, lam, name):
    solver, _, k = name.rpartition("_")
    if solver == "nonnegative":
        return als.ALSEngine(r, f, lam, nonnegative=True)
    return als.ALSEngine(r, f, lam, solver=solver, cg_iters=int(k))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="*", default=[64, 128, 256, 512])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--converge", type=int, nargs="*", default=[])
    ap.add_argument("--conv-iters", type=int, default=10)
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    for f in a.f:
        names = ["block_1", "block_nonneg_1", "block_2", "block_nonneg_2"] + (["nonnegative_0"] if f <= NNLS_MAX_F else [])
        engines = {n: engine(r, f, shp["lam"], n) for n in names}
        print(json.dumps({"shape": a.shape, "f": f, **alternated(engines, a.iters, a.warmup)}), flush=True)
        for eng in engines.values():
            eng.close()
    for f in a.converge:
        live = int((r.csr_indptr.diff() > 0).sum() + (r.csc_indptr.diff() > 0).sum())  # block steps per sweep and block
        for name in ["block_1", "block_nonneg_1"] + (["nonnegative_0"] if f <= NNLS_MAX_F else []):
            eng = engine(r, f, shp["lam"], name)
            eng.init_factors()
            total, elims, seen = 0.0, [], 0
            for _ in range(a.conv_iters):
                total += sum(timed_iteration(eng))
                if name == "block_nonneg_1":
                    failed, now = (int(v) for v in eng.nnls_stats.tolist())
                    elims.append(round((now - seen) / (live * ((f + 31) // 32)), 3))
                    seen = now
            train, test = eng.rmse()
            out = {"shape": a.shape, "f": f, "config": name, "iterations": a.conv_iters, "train_rmse": round(train, 5),
                   "test_rmse": round(test, 5), "ms": round(total, 1)}
            if elims:
                out.update(eliminations_per_block_step=elims, blocks_not_converged=failed)
            print(json.dumps(out), flush=True)
            eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
