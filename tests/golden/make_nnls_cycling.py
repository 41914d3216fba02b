#!/usr/bin/env python3
"""Generate tests/golden/nnls_cycling.npz: 8 x 8 fp32 NNLS systems whose block-principal-pivoting trace from a cold start
reaches Murty's backup rule (tests/nnls_ref.py, nnls_trace).  Random well-conditioned systems almost never do, so the GPU
tests of the pivoting schedule (tests/test_nnls_seams_gpu.py) embed these.  Regenerate with
    python tests/golden/make_nnls_cycling.py
Draw i (seeded by (SEED, i) alone, so that a test can redo one draw):
    k uniform in 1..8, Z a k x 8 standard normal matrix, A = Z^T Z / k + 10^U(-4,-1) I, b standard normal,
    A symmetrised exactly in fp32 as nnls_ref.random_spd does.
It is kept if the fp64 trace of the fp32 system converges, takes at least one Murty step, has a margin >= MARGIN and
cond_2(A) <= COND.  Both thresholds are conditions on the reference: the GPU solver's tolerance is f 2^-24 s <= 7.7e-6 s
for f <= 128, so a margin of 2e-3 is more than 250 times that, and cond_2 <= 2e3 keeps the error of an fp32 elimination
near 1e-4 relative, far inside the margin.
The file holds A, b, the draw numbers, and per case the trace's steps, Murty steps, factorisations, margin and cond_2.  It
is written uncompressed with fixed time stamps, so the same draws give the same bytes.
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import nnls_ref as ref  # noqa: E402

SEED = 20261021
DRAWS = 40000
N = 8
MARGIN = 2e-3
COND = 2e3


def draw(i):
    """(A, b) of draw i, fp32."""
    rng = np.random.RandomState([SEED, i])
    k = rng.randint(1, N + 1)
    Z = rng.standard_normal((k, N))
    A = (Z[:, :, None] * Z[:, None, :]).sum(0) / k + 10.0 ** rng.uniform(-4, -1) * np.eye(N)
    b = rng.standard_normal(N).astype(np.float32)
    A = A.astype(np.float32)
    return 0.5 * (A + A.T), b  # exact in fp32: the two halves are the same value


def accept(A, b):
    """The trace of a draw that meets the conditions, else None."""
    t = ref.nnls_trace(A, b)
    if not t.converged or not any(s.murty for s in t.steps) or t.margin < MARGIN:
        return None
    if np.linalg.cond(A.astype(np.float64), 2) > COND:
        return None
    return t


def write_npz(path, arrays):
    """np.savez without the clock: stored entries with a fixed date, in the given order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as fid:
                np.lib.format.write_array(fid, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)


def main():
    kept = []
    for i in range(DRAWS):
        A, b = draw(i)
        t = accept(A, b)
        if t is not None:
            kept.append((i, A, b, t))
    out = {
        "A": np.stack([k[1] for k in kept]),
        "b": np.stack([k[2] for k in kept]),
        "draw": np.array([k[0] for k in kept], np.int64),
        "steps": np.array([len(k[3].steps) for k in kept], np.int64),
        "murty_steps": np.array([sum(s.murty for s in k[3].steps) for k in kept], np.int64),
        "factorisations": np.array([k[3].factorisations for k in kept], np.int64),
        "margin": np.array([k[3].margin for k in kept], np.float64),
        "cond": np.array([np.linalg.cond(k[1].astype(np.float64), 2) for k in kept], np.float64),
    }
    path = os.path.join(HERE, "nnls_cycling.npz")
    write_npz(path, out)
    print(f"{len(kept)} of {DRAWS} draws kept, {os.path.getsize(path)} bytes")
    for k in ("draw", "steps", "murty_steps", "factorisations"):
        print(k, out[k].tolist())
    print("margin", np.round(out["margin"], 4).tolist())
    print("cond", np.round(out["cond"], 1).tolist())


if __name__ == "__main__":
    main()
