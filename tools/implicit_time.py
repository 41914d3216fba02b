#!/usr/bin/env python3
"""Times implicit-feedback ALS iterations (ImplicitALSEngine) at the Netflix shape: synthetic ratings from
datagen.synth_ratings (17 770 x 480 189, 99 M), alpha = 40, weighted lambda, CG with cg_iters = 3 and LU, f = 64 and 100;
--solver cg_matfree (the operator-only CG) and any even --f up to 512 ("cg" above f = 128 is the same route).
Device-event timing of each half-iteration after warm-up; one JSON line per (f, solver), with the two floors of a
matrix-free half-iteration: the gather, (cg_iters + 1) nnz f 4 B at 6.29 TB/s, and the GEMM work, (cg_iters + 1) x
(2 rows f^2 + 4 nnz f) FLOP at 157.3 TFLOP/s, per side.  Kernel shares come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/implicit_time.py --f 100 --solver lu --iters 2`.
  python tools/implicit_time.py [--f 64 100] [--solver cg lu cg_matfree] [--iters 3] [--warmup 1] [--loss]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100])
    ap.add_argument("--solver", nargs="+", default=["cg", "lu"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--loss", action="store_true", help="also report the objective after each timed iteration")
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    for f in a.f:
        for solver in a.solver:
            if not als.implicit_available(f, "cg_matfree" if solver == "cg" and f > 128 else solver):
                print(json.dumps({"f": f, "solver": solver, "skipped": "not available"}), flush=True)
                continue
            eng = als.ImplicitALSEngine(r, f, shp["lam"], a.alpha, solver=solver, cg_iters=3)
            eng.init_factors()
            eng.iterate(a.warmup)
            torch.cuda.synchronize()
            xs, ts, losses = [], [], []
            for _ in range(a.iters):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                eng.update_x()
                ev[1].record()
                eng.update_theta()
                ev[2].record()
                torch.cuda.synchronize()
                xs.append(ev[0].elapsed_time(ev[1]))
                ts.append(ev[1].elapsed_time(ev[2]))
                if a.loss:
                    losses.append(eng.loss())
            it = sorted(x + t for x, t in zip(xs, ts))
            out = {"shape": a.shape, "f": f, "solver": solver, "alpha": a.alpha, "cg_iters": 3,
                   "ms_per_iter_median": round(it[len(it) // 2], 3), "ms_per_iter_min": round(it[0], 3),
                   "x_ms": [round(v, 3) for v in xs], "theta_ms": [round(v, 3) for v in ts]}
            k = 3 + 1
            out["gather_floor_ms_per_side"] = round(k * shp["nnz"] * f * 4 / 6.29e12 * 1e3, 3)
            out["gemm_floor_ms"] = {side: round(k * (2 * rows * f * f + 4 * shp["nnz"] * f) / 157.3e12 * 1e3, 3)
                                    for side, rows in (("x", shp["m"]), ("theta", shp["n"]))}
            if a.loss:
                out["loss"] = losses
            print(json.dumps(out), flush=True)
            eng.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
