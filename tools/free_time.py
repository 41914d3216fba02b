#!/usr/bin/env python3
"""Times the matrix-free explicit half-iterations (ALSEngine(solver="cg_matfree")) at the Netflix shape against the route
solver="cg" takes at the same f, alternated in one process: synthetic ratings from datagen.synth_ratings (17 770 x 480 189,
99 M), cg_iters = 6, f = 64, 100, 128, 200 (where "cg" is the fused route) and 256, 512 (where it is the generic route that
materialises every f x f system; its batch counts are the smallest that keep a batch of systems under --tt-gb).
Device-event timing of each half-iteration, median of --iters after --warmup; one JSON line per f with the per-side ms of
both routes, their ratio, and the gather floor of a matrix-free half-iteration, (cg_iters + 1) nnz f 4 B at 6.29 TB/s.
A baseline whose warm-up half-iterations took longer than --slow-s seconds is timed once, not --iters times ("reps").
  python tools/free_time.py [--f 64 100 128 200 256 512] [--iters 3] [--warmup 1] [--no-baseline]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402

CG_ITERS = 6


def timed_iteration(eng):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    eng.update_x()
    ev[1].record()
    eng.update_theta()
    ev[2].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def median(v):
    return round(sorted(v)[len(v) // 2], 3)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100, 128, 200, 256, 512])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tt-gb", type=float, default=32.0, help="largest batch of materialised systems of the generic route")
    ap.add_argument("--slow-s", type=float, default=20.0)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    for f in a.f:
        out = {"shape": a.shape, "f": f, "cg_iters": CG_ITERS,
               "gather_floor_ms_per_side": round((CG_ITERS + 1) * shp["nnz"] * f * 4 / 6.29e12 * 1e3, 3)}
        engines = {"cg_matfree": als.ALSEngine(r, f, shp["lam"], solver="cg_matfree", cg_iters=CG_ITERS)}
        if not a.no_baseline:
            fused = bool(als._libmod.load().cumf_fused_available(f, als.SOLVER_CG))
            batches = [1, 1] if fused else [max(1, -(-rows * f * f * 4 // int(a.tt_gb * 1e9))) for rows in (shp["m"], shp["n"])]
            engines["cg"] = als.ALSEngine(r, f, shp["lam"], solver="cg", cg_iters=CG_ITERS, x_batch=batches[0],
                                          theta_batch=batches[1])
            out["baseline"] = {"route": "fused" if fused else "generic", "x_batch": batches[0], "theta_batch": batches[1]}
        reps = {}
        for name, eng in engines.items():
            eng.init_factors()
            t0 = time.time()
            eng.iterate(a.warmup)
            torch.cuda.synchronize()
            reps[name] = 1 if a.warmup and (time.time() - t0) / a.warmup > 2 * a.slow_s else a.iters
            print(f"f={f} {name}: warm-up {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
        times = {name: ([], []) for name in engines}
        for k in range(a.iters):  # alternated
            for name, eng in engines.items():
                if k < reps[name]:
                    x, t = timed_iteration(eng)
                    times[name][0].append(x)
                    times[name][1].append(t)
        for name, (xs, ts) in times.items():
            out[name] = {"x_ms": median(xs), "theta_ms": median(ts), "reps": reps[name],
                         "x_all": [round(v, 3) for v in xs], "theta_all": [round(v, 3) for v in ts]}
        if "cg" in out:
            out["cg_over_matfree"] = {s: round(out["cg"][s] / out["cg_matfree"][s], 3) for s in ("x_ms", "theta_ms")}
        out["matfree_over_floor"] = {s: round(out["cg_matfree"][s] / out["gather_floor_ms_per_side"], 3) for s in ("x_ms", "theta_ms")}
        print(json.dumps(out), flush=True)
        for eng in engines.values():
            eng.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
