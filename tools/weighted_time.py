#!/usr/bin/env python3
"""Times the weighted half-iterations (WeightedALSEngine) at the Netflix shape against the two matrix-free routes they
generalise, as ANOTHER build of the library runs them (the parent commit's libALS.so, built elsewhere and named by --parent):
  weighted, w = 1, w0 = 0                                   against  ALSEngine(solver="cg_matfree")
  weighted, w = 1 + 2 |s|, ratings (s > 0), w0 = 1          against  ImplicitALSEngine(solver="cg_matfree", alpha=2)
with s = rating - 2 (integers -1 .. 3), so that each pair computes the same factors bit for bit and its CGs end at the same
steps.  Synthetic ratings from datagen.synth_ratings (17 770 x 480 189, 99 M), cg_iters = 6, f = 64, 128, 256.

A library is fixed per process (CUMF_ALS_LIB), so the two builds alternate as child processes, --rounds times each
(parent, new, parent, new, ...): every child times all its routes at every f by device events, median of --iters
iterations after --warmup.  One JSON line per (round, library, f); then one summary line per f: per route and side the median
over the rounds, the spread between rounds (max - min over the median), and new / parent.
  python tools/weighted_time.py --parent /path/to/parent/libALS.so [--f 64 128 256] [--rounds 2] [--out FILE.jsonl]"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CG_ITERS, ALPHA = 6, 2.0


def median(v):
    return sorted(v)[len(v) // 2]


def child(role, fs, iters, warmup):
    import torch

    from cumf_als_amd import als, datagen, lib

    if role == "parent":  # a build from before include/cumf_weighted_capi.h: it has none of that header's symbols
        lib.ABI_BY_HEADER.pop("cumf_weighted_capi.h", None)
    shp = datagen.SHAPES["netflix"]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    strength = dataclasses.replace(r, csr_data=r.csr_data - 2.0, csc_data=r.csc_data - 2.0)
    pref = dataclasses.replace(r, csr_data=(strength.csr_data > 0).float(), csc_data=(strength.csc_data > 0).float())
    for f in fs:
        make = {"explicit": lambda: als.ALSEngine(r, f, shp["lam"], solver="cg_matfree", cg_iters=CG_ITERS),
                "implicit": lambda: als.ImplicitALSEngine(strength, f, shp["lam"], ALPHA, solver="cg_matfree", cg_iters=CG_ITERS)}
        if role == "new":
            make["weighted_w0_0"] = lambda: als.WeightedALSEngine(r, torch.ones_like(r.csr_data), f, shp["lam"], w0=0.0,
                                                                  cg_iters=CG_ITERS)
            make["weighted_w0_1"] = lambda: als.WeightedALSEngine(pref, 1 + ALPHA * strength.csr_data.abs(), f, shp["lam"],
                                                                  w0=1.0, cg_iters=CG_ITERS)
        out = {"lib": role, "f": f, "cg_iters": CG_ITERS}
        for name, ctor in make.items():
            eng = ctor()
            eng.init_factors()
            eng.iterate(warmup)
            xs, ts = [], []
            for _ in range(iters):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                eng.update_x()
                ev[1].record()
                eng.update_theta()
                ev[2].record()
                torch.cuda.synchronize()
                xs.append(ev[0].elapsed_time(ev[1]))
                ts.append(ev[1].elapsed_time(ev[2]))
            out[name] = {"x_ms": round(median(xs), 3), "theta_ms": round(median(ts), 3),
                         "x_all": [round(v, 3) for v in xs], "theta_all": [round(v, 3) for v in ts]}
            for p in eng.x_plans + eng.t_plans:  # (not close(): the pooled scratch stays for the next engine)
                p.close()
            del eng
        print(json.dumps(out), flush=True)
    als.release_scratch()
    return 0


def summarise(lines, fs, rounds):
    """One line per f: per library, route and side the median over the rounds and the spread between them, and the ratio of each
    weighted route to the parent's route it generalises."""
    pairs = {"weighted_w0_0": "explicit", "weighted_w0_1": "implicit"}
    out = []
    for f in fs:
        summary = {"summary": True, "f": f, "rounds": rounds}
        stat = {}
        for role in ("parent", "new"):
            for route in ("explicit", "implicit", "weighted_w0_0", "weighted_w0_1"):
                recs = [ln[route] for ln in lines if ln["lib"] == role and ln["f"] == f and route in ln]
                if not recs:
                    continue
                for side in ("x_ms", "theta_ms"):
                    v = [rec[side] for rec in recs]
                    stat[(role, route, side)] = (median(v), (max(v) - min(v)) / median(v))
                summary[f"{role}:{route}"] = {side: {"ms": stat[(role, route, side)][0],
                                                     "spread": round(stat[(role, route, side)][1], 4)}
                                              for side in ("x_ms", "theta_ms")}
        for new, old in pairs.items():
            summary[f"{new}_over_parent_{old}"] = {side: round(stat[("new", new, side)][0] / stat[("parent", old, side)][0], 4)
                                                   for side in ("x_ms", "theta_ms")}
        summary["one_over_f"] = round(1.0 / f, 4)  # the share of the 4 more bytes per entry next to 4 f gathered bytes
        out.append(summary)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build's libALS.so")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=float, default=500.0, help="seconds per child process")
    ap.add_argument("--child", choices=["parent", "new"])
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.f, a.iters, a.warmup)
    if not a.parent or not os.path.exists(a.parent):
        ap.error("--parent must name the other build's libALS.so")
    lines = []
    for rnd in range(a.rounds):
        for role in ("parent", "new"):
            env = dict(os.environ)
            if role == "parent":
                env["CUMF_ALS_LIB"] = os.path.abspath(a.parent)
            else:
                env.pop("CUMF_ALS_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", role, "--iters", str(a.iters), "--warmup", str(a.warmup),
                   "--f"] + [str(f) for f in a.f]
            try:
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"round {rnd} {role}: ran out of time; stopping", file=sys.stderr)
                return 2
            if p.returncode != 0:  # a failed child ends the run: nothing more is started on the device
                print(f"round {rnd} {role}: exit status {p.returncode}; stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 2
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    rec = dict(json.loads(ln), round=rnd)
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
    summaries = summarise(lines, a.f, a.rounds)
    for summary in summaries:
        print(json.dumps(summary), flush=True)
    lines += summaries
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
