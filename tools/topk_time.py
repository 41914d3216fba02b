#!/usr/bin/env python3
"""Times top-k recommendation (als.topk, the fused HIP scoring + selection) at the Netflix shape: synthetic ratings from
datagen.synth_ratings (17 770 x 480 189, 99 M, seed 0), random factors, training entries excluded.  Per (f, k, side): the
device-event ms of cumf_topk, the fp32-MFMA floor 2 rows ncand f / 157.3 TFLOP/s and the fraction of it reached, and the
same job done in torch (chunked fp32 torch.mm, training entries set to -inf, torch.topk) with the share of queries whose
id sets agree, counted over the queries whose k-th and (k+1)-th torch scores are separated.  One JSON line per
configuration.  Kernel shares come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/topk_time.py --no-torch`.
  python tools/topk_time.py [--f 64 100] [--k 10 100] [--side x theta] [--iters 3] [--warmup 1] [--no-torch]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from cumf_als_amd import als, datagen  # noqa: E402

PEAK_FP32_MFMA = 157.3e12  # MI355X fp32 matrix peak, FLOP/s


def torch_topk(query, cand, k, rowptr, colidx, chunk_bytes=4 << 30):
    """(ids, scores) of the unfused route, plus the (k+1)-th score of every query."""
    rows, ncand = query.shape[0], cand.shape[0]
    chunk = max(1, chunk_bytes // (4 * ncand))
    ids = torch.empty((rows, k), dtype=torch.int64, device=query.device)
    scores = torch.empty((rows, k + 1), dtype=torch.float32, device=query.device)
    rp = rowptr.to(torch.int64)
    for a in range(0, rows, chunk):
        b = min(rows, a + chunk)
        s = torch.mm(query[a:b], cand.t())
        lens = rp[a + 1:b + 1] - rp[a:b]
        r = torch.repeat_interleave(torch.arange(b - a, device=query.device), lens)
        s[r, colidx[rp[a]:rp[b]].to(torch.int64)] = float("-inf")
        v, i = torch.topk(s, k + 1, dim=1)
        ids[a:b], scores[a:b] = i[:, :k], v
    return ids, scores


def timed(fn, iters, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return sorted(ms), out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--side", nargs="+", default=["x", "theta"])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="time cumf_topk only (the profiling run)")
    a = ap.parse_args()
    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    for f in a.f:
        g = torch.Generator(device="cpu")
        g.manual_seed(0)
        XT = (0.2 * torch.rand((r.m, f), generator=g)).cuda()
        thetaT = (0.2 * torch.rand((r.n, f), generator=g)).cuda()
        for side in a.side:
            query, cand, seen = ((XT, thetaT, (r.csr_indptr, r.csr_indices)) if side == "x" else
                                 (thetaT, XT, (r.csc_indptr, r.csc_indices)))
            rows, ncand = query.shape[0], cand.shape[0]
            floor_ms = 2.0 * rows * ncand * f / PEAK_FP32_MFMA * 1e3
            for k in a.k:
                ms, (ids, sc) = timed(lambda: als.topk(query, cand, k, seen), a.iters, a.warmup)
                out = {"shape": a.shape, "f": f, "k": k, "side": side, "rows": rows, "ncand": ncand,
                       "topk_ms_median": round(ms[len(ms) // 2], 3), "topk_ms": [round(v, 3) for v in ms],
                       "fp32_mfma_floor_ms": round(floor_ms, 3), "floor_fraction": round(floor_ms / ms[len(ms) // 2], 3)}
                if not a.no_torch:
                    tms, (tids, tsc) = timed(lambda: torch_topk(query, cand, k, *seen), a.iters, a.warmup)
                    sep = (tsc[:, k - 1] - tsc[:, k]) > 1e-5 * tsc[:, k - 1].abs().clamp(min=1.0)
                    same = (torch.sort(ids.to(torch.int64), 1).values == torch.sort(tids, 1).values).all(1)
                    out.update({"torch_ms_median": round(tms[len(tms) // 2], 3),
                                "speedup_vs_torch": round(tms[len(tms) // 2] / ms[len(ms) // 2], 2),
                                "separated_queries": int(sep.sum()),
                                "ids_agree_where_separated": round(float((same & sep).sum()) / max(1, int(sep.sum())), 6)})
                print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
