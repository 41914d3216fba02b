#!/usr/bin/env python3
"""What does the packed partial system cost next to the full one?  On one plan -- the Theta side of the Netflix shape
(synthetic ratings from datagen.synth_ratings: 480 189 systems over 99 M entries) -- the time of
cumf_get_hermitian_implicit_partial (packed upper triangles, no G) against cumf_get_hermitian_implicit (f x f systems with
G; the same device code as before the partial mode existed: tools/kernels_equal.py on als_implicit_kernels.o), the two
alternating, and the time of cumf_implicit_finish on the packed batch.  Device events around each call; the first round
warms up, the median of the others is reported.  One GPU: nothing here says anything about scaling.

Also printed, from the shapes alone: the bytes one rank sends per Theta batch in the reduce-scatter of the `reduce`
scheme, (world - 1) / world of the batch, packed against full.

  python tools/implicit_partial_time.py [--f 64 100] [--rounds 4] [--out profiles/dist_implicit/partial_time.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median(v):
    return sorted(v)[len(v) // 2]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="netflix")
    ap.add_argument("--f", type=int, nargs="+", default=[64, 100])
    ap.add_argument("--rounds", type=int, default=4, help="alternations; the first one warms up")
    ap.add_argument("--world", type=int, default=8, help="ranks of the bytes-per-rank figure")
    ap.add_argument("--out", default=None, help="append every line to this file")
    a = ap.parse_args()
    import torch

    from cumf_als_amd import als, datagen

    shp = datagen.SHAPES[a.shape]
    r = datagen.synth_ratings(shp["m"], shp["n"], shp["nnz"], shp["nnz_test"], seed=0, device="cuda")
    r.csc_data.sub_(2.0)  # interaction strengths with negatives and stored zeros
    lam, alpha = 0.05, 40.0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    lines = []
    for f in a.f:
        rows, pk = r.n, f * (f + 1) // 2
        plan = als.Plan(r.csc_indptr, f)
        g = torch.Generator(device="cpu")
        g.manual_seed(1)
        X = (0.2 * torch.rand((r.m, f), generator=g)).cuda()
        G = als.implicit_gram(X)
        tt = torch.empty((rows, f, f), device="cuda")
        packed = torch.empty((rows, pk), device="cuda")
        rhs = torch.empty((rows, f), device="cuda")
        full_ms, part_ms, fin_ms = [], [], []
        for k in range(a.rounds):
            t_full = timed(lambda: als.get_hermitian_implicit(plan, r.csc_indices, r.csc_data, X, G, lam, alpha, "weighted",
                                                              tt, rhs))
            t_part = timed(lambda: als.get_hermitian_implicit_partial(plan, r.csc_indices, r.csc_data, X, lam, alpha,
                                                                      "weighted", packed, rhs))
            t_fin = timed(lambda: als.implicit_finish(packed, G, 0.0, tt))
            if k:
                full_ms.append(t_full), part_ms.append(t_part), fin_ms.append(t_fin)
        full, part, fin = _median(full_ms), _median(part_ms), _median(fin_ms)
        share = (a.world - 1) / a.world
        line = {"shape": a.shape, "side": "theta", "f": f, "systems": rows, "entries": int(r.csc_indptr[-1].item()),
                "plan_items": plan.n_items, "chunked_rows": plan.n_multi_rows, "rounds_timed": a.rounds - 1,
                "full_ms": round(full, 4), "partial_ms": round(part, 4), "partial_over_full": round(part / full, 4),
                "full_all_ms": [round(v, 4) for v in full_ms], "partial_all_ms": [round(v, 4) for v in part_ms],
                "finish_ms": round(fin, 4), "finish_GB_per_s": round((rows * (pk + f * f) * 4.0) / fin / 1e6, 1),
                "bytes_written_full": rows * f * f * 4, "bytes_written_packed": rows * pk * 4,
                "reduce_scatter_bytes_per_rank": {"world": a.world, "packed": int(share * rows * (pk + f) * 4),
                                                  "full": int(share * rows * (f * f + f) * 4)}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        plan.close()
        del tt, packed, rhs, X
        torch.cuda.empty_cache()
    als.release_scratch()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
