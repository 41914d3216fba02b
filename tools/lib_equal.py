"""Are two builds of the library bit-identical on a half-iteration?
    python tools/lib_equal.py libA libB [f] [solver] [scale] [gram mode] [presplit]
solver: one of ALSEngine's, or implicit:SOLVER:REG for ImplicitALSEngine(solver=SOLVER, alpha=40, reg=REG), e.g.
implicit:cg_matfree:plain (the same factors are hashed; no SSE bins).  Each library runs in its own process (CUMF_ALS_LIB, other CUMF_ALS_* switches inherited), one after the other, for at most
LIB_EQUAL_TIMEOUT seconds (300) each; libB is not started if libA's process failed, died on a signal or ran out of time.  The
factors after two iterations on the Netflix shape (scaled by `scale`) and the fused train-SSE bins of one more Theta update ("-"
where the plans cannot deliver them) are compared bit for bit, and so is the name of the last Gram kernel.  Also printed: the
plans' chunked rows (cumf_plan_info [2]) and the rows of at most 32 ratings, X side / Theta side.  The SSE bins are sums of fp64
atomics: where several rows share a bin their bits can differ between two runs of ONE library
(profiles/r07/route_equal_parent_self.txt).  Exit status: 0 BIT-IDENTICAL, 1 DIFFERENT, 2 a process failed."""
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
if solver.startswith("implicit:"):  # implicit:SOLVER:REG
    eng = als.ImplicitALSEngine(r, f, shp["lam"], 40.0, solver=solver.split(":")[1], reg=solver.split(":")[2])
else:
    eng = als.ALSEngine(r, f, shp["lam"], solver=solver)
eng.init_factors()
eng.iterate(2)
name = als.last_kernel_name().replace(" ", "")
h = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]
sse = "-"
if getattr(eng, "fused", False) and all(als.fused_sse_available(p, solver) for p in eng.t_plans):  # (not the implicit engine)
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
a, b, f, solver, scale, gram, presplit = (sys.argv[1:] + ["100", "lu", "0.3", "auto", "auto"][len(sys.argv) - 3:])[:7]
outs = []
for lib in (a, b):
    env = dict(os.environ, CUMF_ALS_LIB=os.path.join(ROOT, lib))
    try:
        o = subprocess.run([sys.executable, "-c", CHILD, f, solver, scale, gram, presplit], env=env, capture_output=True, text=True,
                           timeout=float(os.environ.get("LIB_EQUAL_TIMEOUT", "300")), check=True)
        outs.append(o.stdout.strip().splitlines()[-1])
    except (subprocess.SubprocessError, IndexError) as e:  # non-zero status, a signal, the time limit, no output
        print(f"{lib}: {type(e).__name__} {getattr(e, 'returncode', '')}; stopping", str(getattr(e, "stderr", ""))[-400:], file=sys.stderr)
        sys.exit(2)
    print(lib, outs[-1])
print("BIT-IDENTICAL" if outs[0].split()[:4] == outs[1].split()[:4] else "DIFFERENT")
sys.exit(outs[0].split()[:4] != outs[1].split()[:4])
