#!/usr/bin/env python3
"""Times the weighted block solver (WeightedALSEngine(solver="block")) at the Netflix shape against the weighted CG with six
steps, alternated iteration by iteration in one process: synthetic ratings from datagen.synth_ratings, weights drawn from
{0.25, 0.5, 1, 2, 4}.  Device-event timing of each half-iteration, median of --iters after --warmup.  One JSON line per
(f, w0) with the X / Theta ms of `cg_6`, `block_1` and `block_2`; --ab F adds the fused Gram route ("auto") against the
segmented one at f = F, w0 = 0.25, one sweep; --converge F adds the loss and the cumulative half-iteration time over
--conv-iters iterations at f = F for the three configurations and both w0.
  python tools/weighted_block_time.py [--f 64 256] [--w0 0 0.25] [--iters 3] [--warmup 1] [--ab 256] [--converge 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402
from tools.block_time import alternated  # noqa: E402
from tools.free_time import timed_iteration  # noqa: E402

CONFIGS = {"cg_6": ("cg", 6), "block_1": ("block", 1), "block_2": ("block", 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="*", default=[64, 256])
    ap.add_argument("--w0", type=float, nargs="*", default=[0.0, 0.25])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ab", type=int, default=0)
    ap.add_argument("--converge", type=int, default=0)
    ap.add_argument("--conv-iters", type=int, default=10)
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    levels = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], device="cuda")
    w = levels[torch.randint(0, 5, r.csr_data.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))]
    make = lambda f, w0, s, k: als.WeightedALSEngine(r, w, f, shp["lam"], w0=w0, solver=s, cg_iters=k)  # noqa: E731
    for f in a.f:
        for w0 in a.w0:
            engines = {name: make(f, w0, s, k) for name, (s, k) in CONFIGS.items()}
            print(json.dumps({"shape": a.shape, "f": f, "w0": w0, **alternated(engines, a.iters, a.warmup)}), flush=True)
            for eng in engines.values():
                eng.close()
    if a.ab:
        engines = {route: make(a.ab, 0.25, "block", 1) for route in ("auto", "segmented")}
        for route, eng in engines.items():
            eng.block_route = route
        print(json.dumps({"shape": a.shape, "f": a.ab, "w0": 0.25, "sweeps": 1,
                          "fused_gram_vs_segmented": alternated(engines, a.iters, a.warmup)}), flush=True)
        for eng in engines.values():
            eng.close()
    if a.converge:
        for w0 in a.w0:
            for name, (s, k) in CONFIGS.items():
                eng = make(a.converge, w0, s, k)
                eng.init_factors()
                total, rows = 0.0, []
                for it in range(a.conv_iters):
                    total += sum(timed_iteration(eng))
                    rows.append({"iteration": it + 1, "loss": eng.loss(), "ms": round(total, 1)})
                print(json.dumps({"shape": a.shape, "f": a.converge, "w0": w0, "config": name, "convergence": rows}), flush=True)
                eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
