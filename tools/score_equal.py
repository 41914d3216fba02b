"""Are two builds of the library bit-identical on the evaluation path (top-k and full ranking)?
    python tools/score_equal.py libA libB [f ...] [--scale 0.3]
The sibling of tools/lib_equal.py for the scoring kernels, with its process rules: each library runs in its own process
(CUMF_ALS_LIB), one after the other, for at most LIB_EQUAL_TIMEOUT seconds (300) each; libB is not started if libA's process
failed, died on a signal or ran out of time.  Per f (default 64: the one-chunk kernels, and 200: the MULTI kernels) and side
of the synthetic Netflix shape scaled by `scale`, random factors, training entries excluded, the generated test set held
out: sha256 of the ids and scores of als.topk at k = 10 and 128, of the ranks and n_eligible of als.heldout_ranks, and the
repr of the outputs of ranking_metrics (on the k = 10 lists) and rank_metrics (cut-offs 10, 100, 1000).
Exit status: 0 BIT-IDENTICAL, 1 DIFFERENT, 2 a process failed."""
import argparse, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, hashlib, torch
sys.path.insert(0, %r)
from cumf_als_amd import als, datagen
scale, fs = float(sys.argv[1]), [int(x) for x in sys.argv[2:]]
shp = datagen.SHAPES["netflix"]
r = datagen.synth_ratings(int(shp["m"] * scale), int(shp["n"] * scale), int(shp["nnz"] * scale * scale),
                          int(shp["nnz_test"] * scale * scale), seed=0, device="cuda")
h = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
for f in fs:
    g = torch.Generator(device="cpu")
    g.manual_seed(0)
    XT = (0.2 * torch.rand((r.m, f), generator=g)).cuda()
    thetaT = (0.2 * torch.rand((r.n, f), generator=g)).cuda()
    for side in ("x", "theta"):
        query, cand, seen, (trow, tcol) = ((XT, thetaT, (r.csr_indptr, r.csr_indices), (r.test_row, r.test_col)) if side == "x"
                                           else (thetaT, XT, (r.csc_indptr, r.csc_indices), (r.test_col, r.test_row)))
        pair = torch.unique((trow.to(torch.int64) << 32) + tcol.to(torch.int64))  # unique within each row
        trow, tcol = (pair >> 32).to(torch.int32), (pair & 0xffffffff).to(torch.int32)
        rowptr, colidx, val = als.heldout_csr(trow, tcol, torch.ones_like(tcol, dtype=torch.float32), query.shape[0])
        out = [f"f={f}", side]
        for k in (10, 128):
            ids, sc = als.topk(query, cand, k, seen)
            out += [h(ids), h(sc)]
            if k == 10:
                m = als.ranking_metrics(ids, rowptr, colidx, val)
        ranks, ne = als.heldout_ranks(query, cand, rowptr, colidx, seen)
        out += [h(ranks), h(ne), repr(m).replace(" ", ""), repr(als.rank_metrics(ranks, ne, rowptr, val, (10, 100, 1000))).replace(" ", "")]
        torch.cuda.synchronize()
        print("RESULT", *out, flush=True)
''' % ROOT
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs=2)
ap.add_argument("f", nargs="*", type=int, default=[64, 200])
ap.add_argument("--scale", default="0.3")
a = ap.parse_args()
outs = []
for lib in a.libs:
    env = dict(os.environ, CUMF_ALS_LIB=os.path.join(ROOT, lib))
    try:
        o = subprocess.run([sys.executable, "-c", CHILD, a.scale] + [str(f) for f in a.f], env=env, capture_output=True, text=True,
                           timeout=float(os.environ.get("LIB_EQUAL_TIMEOUT", "300")), check=True)
        outs.append([l for l in o.stdout.splitlines() if l.startswith("RESULT")])
        if len(outs[-1]) != 2 * len(a.f):
            raise IndexError("missing output")
    except (subprocess.SubprocessError, IndexError) as e:  # non-zero status, a signal, the time limit, no output
        print(f"{lib}: {type(e).__name__} {getattr(e, 'returncode', '')}; stopping", str(getattr(e, "stderr", ""))[-400:], file=sys.stderr)
        sys.exit(2)
    for l in outs[-1]:
        print(lib, l)
print("BIT-IDENTICAL" if outs[0] == outs[1] else "DIFFERENT")
sys.exit(outs[0] != outs[1])
