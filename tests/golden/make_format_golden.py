#!/usr/bin/env python3
"""Generate tests/golden/fmt_ref_loaders.npz: the ten arrays the reference's own loaders
(oracle/_ref/libref_hostutil.so, built by oracle/Makefile when the reference is available)
read from the small dataset of tests/test_format.py.  With it,
test_reference_loaders_read_our_files runs on machines where oracle/_ref cannot be built.
Regenerate with
    python tests/golden/make_format_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from cumf_als_amd import datagen  # noqa: E402
from tests import test_format  # noqa: E402

if __name__ == "__main__":
    import ctypes as C

    if not os.path.exists(test_format.REF_SO):
        raise SystemExit(f"{test_format.REF_SO} is not built (oracle/Makefile needs the reference)")
    r = datagen.synth_ratings(*test_format.DATASET, seed=test_format.DATASET_SEED)
    with tempfile.TemporaryDirectory() as d:
        datagen.write_dataset(r, d)
        ref = test_format._load_with(C.CDLL(test_format.REF_SO), d, r.m, r.n, r.nnz, r.nnz_test)
    out = os.path.join(HERE, "fmt_ref_loaders.npz")
    np.savez_compressed(out, **ref)
    print(out, os.path.getsize(out), "bytes")
