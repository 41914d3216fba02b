#!/usr/bin/env python3
"""Times the weighted half-iterations with rank-one weights on the unstored entries (als.update_weighted_rank1, through
WeightedALSEngine(unobserved=(full(m, 0.3), ones(n)))) and als.weighted_gram at the Netflix shape against what they generalise
as ANOTHER build of the library runs it (the parent commit's libALS.so, built elsewhere and named by --parent):
  WeightedALSEngine(w0 = 0.3) and als.implicit_gram of both factor tables.
The weights w are uniform in [0.5, 4] with a tenth 0 in both.  own = 0.3, gather = 1 computes the factors of w0 = 0.3 bit for
bit, so the CGs end at the same steps; this build times its own w0 = 0.3 route too (the parent's kernels: what a ratio here
can show).  Synthetic ratings from datagen.synth_ratings (17 770 x 480 189, 99 M), cg_iters = 6, f = 64, 128, 256.

A library is fixed per process (CUMF_ALS_LIB), so the two builds alternate as child processes, --rounds times each
(parent, new, parent, new, ...): every child times its routes at every f by device events, median of --iters iterations
after --warmup.  One JSON line per (round, library, f); then one summary line per f: per route and side the median over the
rounds, the spread between rounds (max - min over the median), and new / parent.
  python tools/weighted_rank1_time.py --parent /path/to/parent/libALS.so [--f 64 128 256] [--rounds 2] [--out FILE.jsonl]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CG_ITERS, W0 = 6, 0.3
NEW_SYMBOLS = ("cumf_weighted_gram", "cumf_als_update_weighted_rank1", "cumf_weighted_rank1_loss")


def median(v):
    return sorted(v)[len(v) // 2]


def child(role, fs, iters, warmup):
    import torch

    from cumf_als_amd import als, datagen, lib

    if role == "parent":  # a build from before these entry points
        for sym in NEW_SYMBOLS:
            lib.WEIGHTED_ABI.pop(sym, None)
    shp = datagen.SHAPES["netflix"]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(7)
    w = torch.empty_like(r.csr_data).uniform_(0.5, 4.0, generator=gen)
    w[torch.rand(w.shape, device="cuda", generator=gen) < 0.1] = 0.0
    row_w0 = torch.full((r.m,), W0, dtype=torch.float32, device="cuda")
    col_w0 = torch.ones(r.n, dtype=torch.float32, device="cuda")
    for f in fs:
        make = {"scalar": lambda: als.WeightedALSEngine(r, w, f, shp["lam"], w0=W0, cg_iters=CG_ITERS)}
        if role == "new":
            make["rank1"] = lambda: als.WeightedALSEngine(r, w, f, shp["lam"], cg_iters=CG_ITERS, unobserved=(row_w0, col_w0))
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
            # the Gram of each factor table alone (the X half forms the one of thetaT, the Theta half the one of XT)
            gram = (lambda t, v: als.implicit_gram(t, eng.G)) if name == "scalar" else (lambda t, v: als.weighted_gram(t, v, eng.G))
            for key, table, vec in (("gram_theta_ms", eng.thetaT, col_w0), ("gram_x_ms", eng.XT, row_w0)):
                gs = []
                gram(table, vec)
                for _ in range(5):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    gram(table, vec)
                    ev[1].record()
                    torch.cuda.synchronize()
                    gs.append(ev[0].elapsed_time(ev[1]))
                out[name][key] = round(median(gs), 4)
            for p in eng.x_plans + eng.t_plans:  # (not close(): the pooled scratch stays for the next engine)
                p.close()
            del eng
        print(json.dumps(out), flush=True)
    als.release_scratch()
    return 0


SIDES = ("x_ms", "theta_ms", "gram_theta_ms", "gram_x_ms")


def summarise(lines, fs, rounds):
    """One line per f: per library, route and figure the median over the rounds and the spread between them, and the ratio of
    this build's two routes to the parent's."""
    out = []
    for f in fs:
        summary = {"summary": True, "f": f, "rounds": rounds}
        stat = {}
        for role, route in (("parent", "scalar"), ("new", "scalar"), ("new", "rank1")):
            recs = [ln[route] for ln in lines if ln["lib"] == role and ln["f"] == f and route in ln]
            if not recs:
                continue
            for side in SIDES:
                v = [rec[side] for rec in recs]
                stat[(role, route, side)] = (median(v), (max(v) - min(v)) / median(v))
            summary[f"{role}:{route}"] = {side: {"ms": stat[(role, route, side)][0], "spread": round(stat[(role, route, side)][1], 4)}
                                          for side in SIDES}
        for route in ("scalar", "rank1"):
            if ("new", route, "x_ms") in stat and ("parent", "scalar", "x_ms") in stat:
                summary[f"new_{route}_over_parent_scalar"] = {
                    side: round(stat[("new", route, side)][0] / stat[("parent", "scalar", side)][0], 4) for side in SIDES}
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
