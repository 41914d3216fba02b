#!/usr/bin/env python3
"""Do the explicit and the implicit matrix-free half-iterations of two builds of the library return the same bits?
    python tools/weighted_parent_bits.py PARENT_LIB [NEW_LIB] [--out FILE]
On the seam rows of tests/test_free_gpu.py (its _seam_rows, imported: 45 rows of 0, 1, 7, 8, 9, 15, 16, 17, 2047, 2048, 2049,
4095, 4096, 4097 and short random lengths over 5 000 columns, ratings 0.5 .. 5; the implicit route with signs and stored zeros,
alpha = 2, both reg modes) at f = 10, 254, 510 and cg_iters = 6, and the fp64 implicit objective of each implicit result.  Each
library runs in a process of its own (CUMF_ALS_LIB), one after the other, the second only if the first ended well.  Prints (and
writes to --out) one line per case with both hashes, then SAME or the first difference.
Exit status: 0 SAME, 1 DIFFERENT, 2 a process failed."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FS, CG_ITERS, LAM, ALPHA = (10, 254, 510), 6, 0.05, 2.0


def child():
    import numpy as np
    import torch

    from cumf_als_amd import als, lib
    from tests.test_free_gpu import _seam_rows

    cdll = __import__("ctypes").CDLL(lib.LIB_PATH)
    for table in lib.ABI_BY_HEADER.values():  # a build from before some entry points: none of them is called here
        for sym in [s for s in table if not hasattr(cdll, s)]:
            del table[sym]
    lens, rowptr, colidx, val = _seam_rows()  # the seam case of the tests, not a copy of it
    rng = np.random.RandomState(19)
    signed = (val * rng.choice(np.array([-1.0, 0.0, 1.0, 1.0], np.float32), len(val))).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = {}
    for f in FS:
        Y = dev((0.3 * np.random.RandomState(3).standard_normal((5000, f))).astype(np.float32))
        x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
        plan = als.Plan(rowptr, f)
        x = dev(x0.copy())
        als.update_matfree(plan, dev(colidx), dev(val), Y, x, LAM, CG_ITERS)
        torch.cuda.synchronize()
        out[f"explicit f={f}"] = hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()[:16]
        G = als.implicit_gram(Y)
        for reg in ("weighted", "plain"):
            x = dev(x0.copy())
            als.update_implicit(plan, dev(colidx), dev(signed), Y, G, x, LAM, ALPHA, reg, "cg_matfree", CG_ITERS)
            torch.cuda.synchronize()
            out[f"implicit {reg} f={f}"] = hashlib.sha256(x.cpu().numpy().tobytes()).hexdigest()[:16]
            # the implicit objective of (x, Y): its entry pass is shared with the weighted objective (als_loss.h)
            loss = als.implicit_loss(dev(rowptr), dev(colidx), dev(signed), x, Y, LAM, ALPHA, reg)
            out[f"implicit loss {reg} f={f}"] = loss.cpu().numpy().tobytes().hex()
        plan.close()
    print(json.dumps(out))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("new", nargs="?")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.parent:
        ap.error("name the other build's libALS.so")
    results = []
    for path in (a.parent, a.new):
        env = dict(os.environ)
        env.pop("CUMF_ALS_LIB", None)
        if path:
            env["CUMF_ALS_LIB"] = os.path.abspath(path)
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=300, check=True)
            results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        except (subprocess.SubprocessError, IndexError, ValueError) as e:  # non-zero status, a signal, the time limit, no output
            print(f"{path or 'this build'}: {type(e).__name__} {getattr(e, 'returncode', '')}; stopping",
                  str(getattr(e, "stderr", ""))[-800:], file=sys.stderr)
            return 2
    lines = [f"{case}: parent {results[0][case]} new {results[1][case]}" for case in results[0]]
    diff = [case for case in results[0] if results[0][case] != results[1].get(case)]
    lines.append("SAME" if not diff else f"DIFFERENT: first at {diff[0]}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/weighted_parent_bits.py: the parent commit's libALS.so against this build's, cg_iters = 6\n")
            fh.write("\n".join(lines) + "\n")
    return 1 if diff else 0


if __name__ == "__main__":
    raise SystemExit(main())
