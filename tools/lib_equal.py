"""Are two builds of the library bit-identical on a half-iteration?
    python tools/lib_equal.py libA libB [f] [solver] [scale] [gram mode] [presplit]
Each library runs in its own process (CUMF_ALS_LIB, other CUMF_ALS_* switches inherited); the factors after two iterations on
the Netflix shape (scaled by `scale`) and the fused train-SSE bins of one more Theta update ("-" where the plans cannot
deliver them) are compared bit for bit, and so is the name of the last Gram kernel.  Also printed: the plans' chunked rows
(cumf_plan_info [2]) and the rows of at most 32 ratings, X side / Theta side.  The SSE bins are sums of fp64 atomics: where several
rows share a bin their bits can differ between two runs of ONE library (profiles/r07/route_equal_parent_self.txt)."""
import hashlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %r)
from cumf_als_amd import als, datagen
f, solver, scale, gram, presplit = int(sys.argv[1]), sys.argv[2], float(sys.argv[3]), sys.argv[4], sys.argv[5]
als.set_gram_mode(gram)
als.set_presplit(presplit)
shp = datagen.SHAPES["netflix"]
r = datagen.synth_ratings(int(shp["m"] * scale), int(shp["n"] * scale), int(shp["nnz"] * scale * scale), 1000, seed=0, device="cuda")
eng = als.ALSEngine(r, f, shp["lam"], solver=solver)
eng.init_factors()
eng.iterate(2)
name = als.last_kernel_name().replace(" ", "")
h = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
sse = "-"
if eng.fused and all(als.fused_sse_available(p, solver) for p in eng.t_plans):
    bins = torch.zeros(als.SSE_BINS, dtype=torch.float64, device="cuda")
    for p in eng.t_plans:
        als.update_fused_sse(p, r.csc_indices, r.csc_data, eng.XT, eng.thetaT, eng.lam, solver, eng.cg_iters, bins)
    sse = h(bins)
torch.cuda.synchronize()
short = lambda rp: int(((rp[1:] - rp[:-1]) <= 32).sum())
facts = "chunked {}/{} short {}/{}".format(sum(p.n_multi_rows for p in eng.x_plans), sum(p.n_multi_rows for p in eng.t_plans),
                                          short(r.csr_indptr.cpu().numpy()), short(r.csc_indptr.cpu().numpy()))
print(h(eng.XT), h(eng.thetaT), sse, name, facts)
''' % ROOT
a, b = sys.argv[1], sys.argv[2]
f = sys.argv[3] if len(sys.argv) > 3 else "100"
solver = sys.argv[4] if len(sys.argv) > 4 else "lu"
scale = sys.argv[5] if len(sys.argv) > 5 else "0.3"
gram = sys.argv[6] if len(sys.argv) > 6 else "auto"
presplit = sys.argv[7] if len(sys.argv) > 7 else "auto"
outs = []
for lib in (a, b):
    env = dict(os.environ, CUMF_ALS_LIB=os.path.join(ROOT, lib))
    o = subprocess.run([sys.executable, "-c", CHILD, f, solver, scale, gram, presplit], env=env, capture_output=True, text=True)
    line = [l for l in o.stdout.splitlines() if l.strip()][-1] if o.stdout.strip() else o.stderr[-400:]
    outs.append(line)
    print(lib, line)
print("BIT-IDENTICAL" if outs[0].split()[:4] == outs[1].split()[:4] else "DIFFERENT")
