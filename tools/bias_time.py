#!/usr/bin/env python3
"""What do the bias terms cost?  Step time of BiasedALSEngine(f = 98, "lu") -- F = 100, the kernel instances of the headline
-- against ALSEngine(f = 100, "lu") of the PARENT commit's library, at the Netflix shape (synthetic ratings from
datagen.synth_ratings: 17 770 x 480 189, 99 M).

Each measurement is a fresh process (the plain side imports cumf_als_amd, library included, from a built checkout of the
parent commit: --parent-tree), the two sides alternate, and every process reports the median over its timed steps; the
result is the median of the processes' medians (3 per side by default).  A step is one X half plus one Theta half, timed with device events around each half; iterations 1 and 2 warm up.
The biased process also times the residual kernel alone (cumf_bias_residual on the CSR arrays, 12 bytes per rating) and
reports its share of the 6.3 TB/s a streaming kernel reaches on this GPU.

  python tools/bias_time.py --parent-tree PARENT_CHECKOUT [--out profiles/bias/bias_time.jsonl]
  python tools/bias_time.py --one biased|plain        one process, one JSON line (what the driver starts)

Without --parent-tree the plain side runs on this tree's library (the training kernels are the same device code:
tools/kernels_equal.py), and the line says so."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_ACHIEVABLE = 6.3e12  # bytes/s, float4 copy on one MI355X


def _median(v):
    return sorted(v)[len(v) // 2]


def one(kind, a):
    sys.path.insert(0, os.path.abspath(a.parent_tree) if kind == "plain" and a.parent_tree else ROOT)
    import torch

    from cumf_als_amd import als, datagen, lib

    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    lam = shp["lam"]
    if kind == "biased":
        e = als.BiasedALSEngine(r, a.f, lam, solver="lu")
    else:
        e = als.ALSEngine(r, a.f + 2, lam, solver="lu")
    e.init_factors()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    xs, ts = [], []
    for it in range(a.warmup + a.steps):
        ev[0].record()
        e.update_x()
        ev[1].record()
        e.update_theta()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            xs.append(ev[0].elapsed_time(ev[1]))
            ts.append(ev[1].elapsed_time(ev[2]))
    out = {"kind": kind, "lib": lib.LIB_PATH, "shape": a.shape, "f": a.f if kind == "biased" else a.f + 2, "F": a.f + 2,
           "steps": a.steps, "x_ms": round(_median(xs), 4), "theta_ms": round(_median(ts), 4),
           "step_ms": round(_median([x + t for x, t in zip(xs, ts)]), 4), "kernel": als.last_kernel_name(),
           "rmse": [round(v, 6) for v in e.rmse()]}
    if kind == "biased":
        # the residual kernel alone, both sides' arrays: 12 bytes per rating (val, colidx read, r' written)
        res = {}
        for side, val, idx, bias in (("x", r.csr_data, r.csr_indices, e.item_bias), ("theta", r.csc_data, r.csc_indices,
                                                                                     e.user_bias)):
            dst = torch.empty_like(val)
            ms = []
            for k in range(3 + 15):
                ev[0].record()
                als.residual_biased(val, idx, bias, e.mu, dst)
                ev[1].record()
                torch.cuda.synchronize()
                if k >= 3:
                    ms.append(ev[0].elapsed_time(ev[1]))
            t = _median(ms)
            bytes_ = 12.0 * val.numel()
            res[side] = {"ms": round(t, 4), "GB_per_s": round(bytes_ / t / 1e6, 1),
                         "share_of_achievable_hbm": round(bytes_ / (t * 1e-3) / HBM_ACHIEVABLE, 3)}
            del dst
        out["residual_kernel"] = res
        out["floor_ms_per_side"] = round(12.0 * r.nnz / HBM_ACHIEVABLE * 1e3, 4)
    e.close()
    print(json.dumps(out), flush=True)
    return 0


def drive(a):
    me = os.path.abspath(__file__)
    runs = {"biased": [], "plain": []}
    for _ in range(a.processes):
        for kind in ("plain", "biased"):
            env = dict(os.environ)
            env.pop("CUMF_ALS_LIB", None)
            cmd = [sys.executable, me, "--one", kind, "--shape", a.shape, "--f", str(a.f), "--steps", str(a.steps),
                   "--warmup", str(a.warmup)] + (["--parent-tree", a.parent_tree] if a.parent_tree else [])
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.stderr.write(p.stdout + p.stderr)
                return p.returncode or 1
            line = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            runs[kind].append(line)
    med = {k: {q: _median([r[q] for r in v]) for q in ("x_ms", "theta_ms", "step_ms")} for k, v in runs.items()}
    over = med["biased"]["step_ms"] - med["plain"]["step_ms"]
    b0 = runs["biased"][0]
    summary = {"summary": "bias_time", "shape": a.shape, "f": a.f, "F": a.f + 2, "processes_per_side": a.processes,
               "plain_library": "parent" if a.parent_tree else "this tree", "plain": med["plain"], "biased": med["biased"],
               "overhead_ms": round(over, 4), "overhead_share_of_step": round(over / med["plain"]["step_ms"], 4),
               "overhead_x_ms": round(med["biased"]["x_ms"] - med["plain"]["x_ms"], 4),
               "overhead_theta_ms": round(med["biased"]["theta_ms"] - med["plain"]["theta_ms"], 4),
               "floor_ms_per_side": b0["floor_ms_per_side"],
               "residual_kernel": {s: {q: _median([r["residual_kernel"][s][q] for r in runs["biased"]])
                                       for q in ("ms", "GB_per_s", "share_of_achievable_hbm")} for s in ("x", "theta")},
               "plain_step_spread": [min(r["step_ms"] for r in runs["plain"]), max(r["step_ms"] for r in runs["plain"])],
               "biased_step_spread": [min(r["step_ms"] for r in runs["biased"]), max(r["step_ms"] for r in runs["biased"])]}
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in runs["plain"] + runs["biased"] + [summary]:
                fh.write(json.dumps(line) + "\n")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, default=98, help="factors of the biased model; the plain engine runs at f + 2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--processes", type=int, default=3, help="fresh processes per side, alternating")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (the plain side imports it)")
    ap.add_argument("--timeout", type=float, default=280.0, help="seconds per process")
    ap.add_argument("--one", choices=("biased", "plain"), default=None)
    ap.add_argument("--out", default=None, help="append every line to this file")
    a = ap.parse_args()
    return one(a.one, a) if a.one else drive(a)


if __name__ == "__main__":
    raise SystemExit(main())
