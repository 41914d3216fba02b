#!/usr/bin/env python3
"""Times non-negative ALS (nonnegative=True engines) at the Netflix shape: synthetic ratings from datagen.synth_ratings
(17 770 x 480 189, 99 M), f = 64 and 100, explicit (lambda = 0.048) and implicit (alpha = 40, weighted lambda).
Iteration 1 (from x = 0, theta random >= 0) is the warm-up; iterations 2 .. 1 + iters are timed with device events per
half-iteration.  Per (f, model) one JSON line with:
  * ms per half-iteration (X side, Theta side), median and per iteration;
  * passive-set factorisations per row (nnls_stats deltas / rows) and the largest step count of any row, at iterations
    1, 2, 5 and 10 (the largest is probed before the half-iteration on the same systems and warm start: the smallest
    max_iters that leaves no row unconverged);
  * after the last iteration, on the Theta side's materialised batch: nnls_solve (warm start from the current factors,
    and cold from 0) against cumf_lu_solve_batched, ms per factorisation against ms per LU system;
  * train / test RMSE (explicit) or the objective (implicit) after 10 iterations, non-negative and unconstrained LU.
The split of a half-iteration into materialise / NNLS kernel / rest comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/nnls_time.py --iters 2 --no-probe --no-baseline`, whose kernel trace
`--split TRACE.csv` turns into kernel ms per half-iteration (iteration 3 of each configuration, in the default order).
  python tools/nnls_time.py [--f 64 100] [--model explicit implicit] [--iters 10]
  python tools/nnls_time.py --split nnls_kernel_trace.csv"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402

PROBE_AT = (1, 2, 5, 10)


def _engine(r, f, model, lam, alpha, nonneg):
    if model == "explicit":
        e = als.ALSEngine(r, f, lam, solver="lu", nonnegative=nonneg)
    else:
        e = als.ImplicitALSEngine(r, f, lam, alpha, solver="lu", nonnegative=nonneg)
    e.init_factors()
    return e


def _systems(e, model, side, tt=None, rhs=None):
    """The materialised systems of one side's (single) plan for the current factors."""
    r = e.r
    plan, colidx, val, gather = ((e.x_plans[0], r.csr_indices, r.csr_data, e.thetaT) if side == "x" else
                                 (e.t_plans[0], r.csc_indices, r.csc_data, e.XT))
    if model == "explicit":
        return als.get_hermitian(plan, colidx, val, gather, e.lam, tt, rhs)
    return als.get_hermitian_implicit(plan, colidx, val, gather, als.implicit_gram(gather), e.lam, e.alpha, e.reg, tt,
                                      rhs)


def _max_steps(A, b, x0, cap=64):
    """Smallest max_iters with no unconverged row (solves on a copy of the warm start)."""
    st = torch.zeros(2, dtype=torch.int64, device=A.device)
    for k in range(1, cap + 1):
        st.zero_()
        als.nnls_solve(A, b, x0.clone(), k, st)
        if int(st[0].item()) == 0:
            return k
    return None


def _timed(fn, reps=3):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    return sorted(ts)[len(ts) // 2]


def run(r, shp, f, model, a):
    lam = shp["lam"]
    e = _engine(r, f, model, lam, a.alpha, True)
    bufs = {}
    xs, ts, counts = [], [], {}
    for it in range(1, a.iters + 2):
        row = {}
        for side, half, rows, table in (("x", e.update_x, e.m, lambda: e.XT), ("theta", e.update_theta, e.n,
                                                                                 lambda: e.thetaT)):
            if not a.no_probe and it in PROBE_AT:
                tt, rhs = bufs.get(side, (None, None))
                tt, rhs = _systems(e, model, side, tt, rhs)
                bufs[side] = (tt, rhs)
                row[f"{side}_max_steps"] = _max_steps(tt, rhs, table())
            before = e.nnls_stats.clone()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            half()
            ev[1].record()
            torch.cuda.synchronize()
            d = (e.nnls_stats - before).tolist()
            row[f"{side}_fact_per_row"] = round(d[1] / rows, 4)
            row[f"{side}_unconverged"] = d[0]
            if it > 1:
                (xs if side == "x" else ts).append(ev[0].elapsed_time(ev[1]))
        if it in PROBE_AT:
            counts[it] = row
    out = {"shape": a.shape, "f": f, "model": model, "lam": lam, "alpha": a.alpha if model == "implicit" else None,
           "iters_timed": a.iters, "x_ms_median": round(sorted(xs)[len(xs) // 2], 3),
           "theta_ms_median": round(sorted(ts)[len(ts) // 2], 3), "x_ms": [round(v, 3) for v in xs],
           "theta_ms": [round(v, 3) for v in ts], "per_iteration": counts, "nnls_stats": e.nnls_stats.tolist()}
    # the NNLS kernel against the batched LU on the same materialised batch (Theta side, current factors)
    tt, rhs = bufs.get("theta", (None, None))
    tt, rhs = _systems(e, model, "theta", tt, rhs)
    bufs.clear()
    n = rhs.shape[0]
    st = torch.zeros(2, dtype=torch.int64, device=rhs.device)
    x_lu = torch.empty_like(rhs)
    for start, x0 in (("warm", e.thetaT), ("cold", torch.zeros_like(rhs))):
        x = x0.clone()
        st.zero_()
        als.nnls_solve(tt, rhs, x, 0, st)  # warm-up + the factorisation count of one call
        torch.cuda.synchronize()
        facts = int(st[1].item())
        ms = _timed(lambda: als.nnls_solve(tt, rhs, x0.clone(), 0))
        out[f"theta_batch_nnls_{start}"] = {"systems": n, "ms": round(ms, 3), "factorisations": facts,
                                             "fact_per_system": round(facts / n, 4),
                                             "us_per_factorisation": round(1e3 * ms / max(facts, 1), 5)}
    # the clone of the warm start is part of the timed call above: time it alone and report it
    out["theta_batch_clone_ms"] = round(_timed(lambda: e.thetaT.clone()), 3)
    als.lu_solve(tt, rhs, x_lu)
    ms_lu = _timed(lambda: als.lu_solve(tt, rhs, x_lu))
    out["theta_batch_lu"] = {"systems": n, "ms": round(ms_lu, 3), "us_per_system": round(1e3 * ms_lu / n, 5)}
    for start in ("warm", "cold"):
        nn = out[f"theta_batch_nnls_{start}"]
        per_fact = (nn["ms"] - out["theta_batch_clone_ms"]) / max(nn["factorisations"], 1)
        out[f"theta_batch_nnls_{start}"]["per_factorisation_over_lu_per_system"] = round(per_fact / (ms_lu / n), 3)
    del tt, rhs
    if model == "explicit":
        out["rmse_nonneg"] = e.rmse()
    else:
        out["loss_nonneg"] = e.loss()
    out["min_factor"] = min(float(e.XT.min()), float(e.thetaT.min()))
    e.close()
    if not a.no_baseline:
        b = _engine(r, f, model, lam, a.alpha, False)
        b.iterate(a.iters + 1)
        torch.cuda.synchronize()
        if model == "explicit":
            out["rmse_lu"] = b.rmse()
        else:
            out["loss_lu"] = b.loss()
        b.close()
    return out


def split(trace, fs=(64, 100), models=("explicit", "implicit"), iters=2):
    """Kernel ms of each half-iteration in a kernel trace of `--iters 2 --no-probe --no-baseline`: the kernels since the
    previous NNLS dispatch are attributed to the next one.  Per configuration the tool dispatches 2 (iters + 1) halves, then
    8 NNLS calls on the Theta batch; the last timed iteration's two halves are printed."""
    def kind(name):
        if "nnls_bpp_kernel" in name:
            return "nnls"
        if "implicit_gram" in name:
            return "gram"
        if "implicit_zero_rows" in name:
            return "zero_rows"
        if any(k in name for k in ("als_wave", "als_item", "als_reduce", "implicit_hermitian", "implicit_slot_reduce")):
            return "materialise"
        return None
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
    halves, acc = [], {}
    for r in rows:
        k = kind(r["Kernel_Name"])
        if k is None:
            continue
        acc[k] = acc.get(k, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if k == "nnls":
            halves.append({key: round(v, 3) for key, v in acc.items()})
            acc = {}
    per = 2 * (iters + 1) + 8
    configs = [(f, m) for f in fs for m in models]
    for i, (f, m) in enumerate(configs):
        h = halves[per * i: per * (i + 1)]
        for j, side in ((2 * iters, "x"), (2 * iters + 1, "theta")):
            print(json.dumps({"f": f, "model": m, "iteration": iters + 1, "side": side, "kernel_ms": h[j]}))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100])
    ap.add_argument("--model", nargs="+", default=["explicit", "implicit"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--no-probe", action="store_true", help="skip the largest-step probes")
    ap.add_argument("--no-baseline", action="store_true", help="skip the unconstrained LU engines")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--split", metavar="TRACE", default=None, help="print the kernel split of a rocprofv3 kernel trace")
    a = ap.parse_args()
    if a.split:
        split(a.split, tuple(a.f), tuple(a.model), a.iters if a.iters != 10 else 2)
        return 0
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    for f in a.f:
        for model in a.model:
            line = json.dumps(run(r, shp, f, model, a))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
