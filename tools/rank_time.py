#!/usr/bin/env python3
"""Times full-ranking evaluation (als.heldout_ranks: the fused HIP scoring + a count per held-out threshold) at the Netflix
shape: synthetic ratings from datagen.synth_ratings (17 770 x 480 189, 99 M, seed 0), random factors, the generated test set
held out (made unique per row), training entries excluded.  Per (f, side): the device-event ms of cumf_heldout_ranks and, in
the same process and alternated with it, of cumf_topk at k = 100 (the same MFMA work with a heavier consumer: the
yardstick) with their ratio; the fp32-MFMA floor 2 rows ncand f / 157.3 TFLOP/s and the fraction of it reached; the ms of
cumf_rank_metrics; and the same ranks done in torch (chunked fp32 torch.mm, training entries set to -inf, gather of the
held-out scores, compare-and-sum) with the share of entries whose rank agrees where no other score ties with theirs to
1e-5.  One JSON line per configuration.  Kernel shares come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/rank_time.py --no-torch`.
  python tools/rank_time.py [--f 64 100] [--side x theta] [--iters 3] [--warmup 1] [--no-torch]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402

PEAK_FP32_MFMA = 157.3e12  # MI355X fp32 matrix peak, FLOP/s


def torch_ranks(query, cand, rowptr, colidx, trowptr, tcolidx, chunk_bytes=4 << 30):
    """ranks by score alone (ties not broken by index) of the unfused route, and the count of scores within 1e-5 of each
    held-out score (1 = only its own)."""
    rows, ncand = query.shape[0], cand.shape[0]
    chunk = max(1, chunk_bytes // (4 * ncand))
    ranks = torch.empty(tcolidx.shape[0], dtype=torch.int64, device=query.device)
    near = torch.empty_like(ranks)
    rp, tp = rowptr.to(torch.int64), trowptr.to(torch.int64)
    sub = max(1, (1 << 30) // ncand)  # held-out entries compared at a time
    for a in range(0, rows, chunk):
        b = min(rows, a + chunk)
        s = torch.mm(query[a:b], cand.t())
        r = torch.repeat_interleave(torch.arange(b - a, device=query.device), rp[a + 1:b + 1] - rp[a:b])
        s[r, colidx[rp[a]:rp[b]].to(torch.int64)] = float("-inf")
        e0, e1 = int(tp[a]), int(tp[b])
        tr = torch.repeat_interleave(torch.arange(b - a, device=query.device), tp[a + 1:b + 1] - tp[a:b])
        st = s[tr, tcolidx[e0:e1].to(torch.int64)]
        for x in range(0, e1 - e0, sub):
            y = min(e1 - e0, x + sub)
            row = s[tr[x:y]]
            ranks[e0 + x:e0 + y] = (row > st[x:y, None]).sum(1)
            near[e0 + x:e0 + y] = ((row - st[x:y, None]).abs() <= 1e-5 * st[x:y, None].abs().clamp(min=1.0)).sum(1)
    return ranks, near


def timed(fns, iters, warmup):
    """Sorted device-event ms of each of fns, alternated: one call of each per round."""
    ms = [[] for _ in fns]
    out = [None] * len(fns)
    for it in range(warmup + iters):
        for i, fn in enumerate(fns):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            out[i] = fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[i].append(ev[0].elapsed_time(ev[1]))
    return [sorted(m) for m in ms], out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100])
    ap.add_argument("--side", nargs="+", default=["x", "theta"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="time the library only (the profiling run)")
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    med = lambda m: round(m[len(m) // 2], 3)  # noqa: E731
    for f in a.f:
        g = torch.Generator(device="cpu")
        g.manual_seed(0)
        XT = (0.2 * torch.rand((r.m, f), generator=g)).cuda()
        thetaT = (0.2 * torch.rand((r.n, f), generator=g)).cuda()
        for side in a.side:
            query, cand, seen, (trow, tcol) = ((XT, thetaT, (r.csr_indptr, r.csr_indices), (r.test_row, r.test_col)) if side == "x"
                                               else (thetaT, XT, (r.csc_indptr, r.csc_indices), (r.test_col, r.test_row)))
            rows, ncand = query.shape[0], cand.shape[0]
            pair = torch.unique((trow.to(torch.int64) << 32) + tcol.to(torch.int64))  # unique within each row
            trow, tcol = (pair >> 32).to(torch.int32), (pair & 0xffffffff).to(torch.int32)
            rowptr, colidx, val = als.heldout_csr(trow, tcol, torch.ones_like(tcol, dtype=torch.float32), rows)
            floor_ms = 2.0 * rows * ncand * f / PEAK_FP32_MFMA * 1e3
            (rms, tms), ((ranks, ne), _) = timed([lambda: als.heldout_ranks(query, cand, rowptr, colidx, seen),
                                                  lambda: als.topk(query, cand, 100, seen)], a.iters, a.warmup)
            (mms,), (metrics,) = timed([lambda: als.rank_metrics(ranks, ne, rowptr, val, (10, 100, 1000))], a.iters, a.warmup)
            out = {"shape": a.shape, "f": f, "side": side, "rows": rows, "ncand": ncand, "heldout": int(colidx.shape[0]),
                   "longest_heldout_row": int((rowptr[1:] - rowptr[:-1]).max()),
                   "ranks_ms_median": med(rms), "ranks_ms": [round(v, 3) for v in rms],
                   "topk100_ms_median": med(tms), "topk100_ms": [round(v, 3) for v in tms],
                   "ranks_over_topk100": round(med(rms) / med(tms), 3),
                   "fp32_mfma_floor_ms": round(floor_ms, 3), "floor_fraction": round(floor_ms / med(rms), 3),
                   "metrics_ms_median": med(mms), "mpr": round(metrics["mpr"], 6), "auc": round(metrics["auc"], 6)}
            if not a.no_torch:
                (qms,), ((tr, near),) = timed([lambda: torch_ranks(query, cand, *seen, rowptr, colidx)], 1, 0)
                ok = (ranks >= 0) & (near == 1)
                out.update({"torch_ms": med(qms), "speedup_vs_torch": round(med(qms) / med(rms), 2),
                            "untied_entries": int(ok.sum()),
                            "ranks_agree_where_untied": round(float((ranks.to(torch.int64) == tr)[ok].sum()) / max(1, int(ok.sum())), 6)})
            print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
