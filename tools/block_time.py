#!/usr/bin/env python3
"""Times the explicit block solver (ALSEngine(solver="block")) at the Netflix shape against the matrix-free CG with six steps,
alternated iteration by iteration in one process: synthetic ratings from datagen.synth_ratings (17 770 x 480 189, 99 M).
Device-event timing of each half-iteration, median of --iters after --warmup.  One JSON line per f with the X / Theta ms of
`cg_matfree` (6 steps), `block` with 1 and 2 sweeps and their gather floors, (1 + 2 sweeps) resp. (cg_iters + 1) nnz f 4 B at
6.29 TB/s; --ab F adds the fused route against the segmented one at f = F, one sweep; --converge F adds train / test RMSE and
cumulative half-iteration time over --conv-iters iterations at f = F for the three configurations.
  python tools/block_time.py [--f 64 128 256 512] [--iters 3] [--warmup 1] [--ab 256] [--converge 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402
from tools.free_time import median, timed_iteration  # noqa: E402

CONFIGS = {"cg_matfree_6": ("cg_matfree", 6), "block_1": ("block", 1), "block_2": ("block", 2)}


def alternated(engines, iters, warmup):
    for eng in engines.values():
        eng.init_factors()
        eng.iterate(warmup)
    times = {name: ([], []) for name in engines}
    for _ in range(iters):
        for name, eng in engines.items():
            x, t = timed_iteration(eng)
            times[name][0].append(x)
            times[name][1].append(t)
    return {name: {"x_ms": median(xs), "theta_ms": median(ts), "x_all": [round(v, 3) for v in xs],
                   "theta_all": [round(v, 3) for v in ts]} for name, (xs, ts) in times.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="*", default=[64, 128, 256, 512])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ab", type=int, default=0)
    ap.add_argument("--converge", type=int, default=0)
    ap.add_argument("--conv-iters", type=int, default=10)
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    floor = lambda passes, f: round(passes * shp["nnz"] * f * 4 / 6.29e12 * 1e3, 3)  # noqa: E731
    for f in a.f:
        engines = {name: als.ALSEngine(r, f, shp["lam"], solver=s, cg_iters=k) for name, (s, k) in CONFIGS.items()}
        out = {"shape": a.shape, "f": f, **alternated(engines, a.iters, a.warmup),
               "gather_floor_ms_per_side": {"cg_matfree_6": floor(7, f), "block_1": floor(3, f), "block_2": floor(5, f)}}
        print(json.dumps(out), flush=True)
        for eng in engines.values():
            eng.close()
    if a.ab:
        engines = {route: als.ALSEngine(r, a.ab, shp["lam"], solver="block", cg_iters=1) for route in ("auto", "segmented")}
        for route, eng in engines.items():
            eng.block_route = route
        print(json.dumps({"shape": a.shape, "f": a.ab, "sweeps": 1, "fused_vs_segmented": alternated(engines, a.iters, a.warmup)}),
              flush=True)
        for eng in engines.values():
            eng.close()
    if a.converge:
        for name, (s, k) in CONFIGS.items():
            eng = als.ALSEngine(r, a.converge, shp["lam"], solver=s, cg_iters=k)
            eng.init_factors()
            total, rows = 0.0, []
            for it in range(a.conv_iters):
                total += sum(timed_iteration(eng))
                train, test = eng.rmse()
                rows.append({"iteration": it + 1, "train_rmse": round(train, 5), "test_rmse": round(test, 5), "ms": round(total, 1)})
            print(json.dumps({"shape": a.shape, "f": a.converge, "config": name, "convergence": rows}), flush=True)
            eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
