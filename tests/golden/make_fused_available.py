"""Writes fused_available.json: cumf_fused_available(f, solver) for f = 1 .. 520 under each gram mode, as a string of
0 / 1 per (gram mode, solver).  Run once against the library whose answers the table pins:

    python tests/golden/make_fused_available.py path/to/libALS.so
"""
import ctypes as C
import json
import os
import sys

GRAM_MODES = {"auto": 0, "exact": 1, "fast": 2}  # CUMF_GRAM_*
SOLVERS = {"cg": 0, "lu": 1}                     # CUMF_SOLVER_*
F_MAX = 520


def table(lib):
    out = {}
    for gname, g in GRAM_MODES.items():
        assert lib.cumf_set_gram_mode(g) == 0
        out[gname] = {s: "".join(str(lib.cumf_fused_available(f, sid)) for f in range(1, F_MAX + 1))
                      for s, sid in SOLVERS.items()}
    lib.cumf_set_gram_mode(0)
    return out


if __name__ == "__main__":
    lib = C.CDLL(os.path.abspath(sys.argv[1]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fused_available.json")
    with open(path, "w") as fh:
        json.dump(table(lib), fh, indent=1)
        fh.write("\n")
