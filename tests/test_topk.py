"""Top-k recommendation without a GPU: the C ABI of include/cumf_topk_capi.h is exported and listed, its scope check, and
self-checks of the numpy reference that tests/test_topk_gpu.py measures against."""
import os
import re
from fractions import Fraction

import numpy as np

from tests import topk_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topk_header_symbols_are_exported(alslib):
    from cumf_als_amd import lib

    text = open(os.path.join(ROOT, "include", "cumf_topk_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cumf_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared and set(declared) == set(lib.TOPK_SYMBOLS), (declared, lib.TOPK_SYMBOLS)
    for s in declared:
        assert hasattr(alslib, s), s


def test_topk_available_table(alslib):
    for f in (0, 1, 512, 513):
        for k in (0, 1, 128, 129):
            want = int(1 <= f <= 512 and 1 <= k <= 128)
            assert alslib.cumf_topk_available(f, k) == want, (f, k)


def test_reference_chain_is_fmaf_on_dyadic_data():
    rng = np.random.RandomState(0)
    Q, C = ref.dyadic(rng, (3, 37)), ref.dyadic(rng, (5, 37))
    s = ref.chain_scores(Q, C)
    for q in range(3):
        for c in range(5):
            acc = Fraction(0)
            for j in range(37):  # fmaf: the exact q c + s, rounded once to fp32 (exact in fp64 on dyadic data)
                v = acc + Fraction(float(Q[q, j])) * Fraction(float(C[c, j]))
                assert Fraction(float(v)) == v
                acc = Fraction(float(np.float32(float(v))))
            assert s[q, c] == np.float32(float(acc))
    # zero padding of the features does not change the chain
    Qp = np.concatenate([Q, np.zeros((3, 3), np.float32)], 1)
    Cp = np.concatenate([C, np.zeros((5, 3), np.float32)], 1)
    assert np.array_equal(ref.chain_scores(Qp, Cp).view(np.int32), s.view(np.int32))


def test_reference_topk_ties_nan_exclusion_padding():
    s = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 2.0, 3.0]], np.float32)
    ids, sc = ref.topk(s, 5)
    assert ids.tolist() == [[1, 3, 6, 5, 0]] and sc.tolist() == [[3.0, 3.0, 3.0, 2.0, 1.0]]
    ids, sc = ref.topk(s, 8, exclude=[[3, 3, 5]])  # duplicates allowed; fewer eligible than k: -1 / -inf
    assert ids.tolist() == [[1, 6, 0, 4, -1, -1, -1, -1]]
    assert sc[0, 3] == -np.inf and np.all(sc[0, 4:] == -np.inf)
    ids, _ = ref.topk(s, 2, exclude=[list(range(7))])
    assert ids.tolist() == [[-1, -1]]


def test_reference_ndcg_hand_computed():
    # one query, k = 3, list (5, 2, 9), relevant {2, 9, 11, 40}: hits at positions 1 and 2
    ids = np.array([[5, 2, 9], [1, -1, -1], [4, 4, 4]], np.int32)
    rowptr = np.array([0, 4, 5, 6])
    colidx = np.array([2, 9, 11, 40, 1, 4])
    val = np.array([1.0, 2.0, 0.5, 1.0, 3.0, -1.0], np.float32)  # row 2: nothing relevant
    n, p, r, g = ref.ranking_metrics(ids, rowptr, colidx, val)
    dcg0 = 1 / np.log2(3) + 1 / np.log2(4)
    idcg0 = 1 + 1 / np.log2(3) + 1 / np.log2(4)
    assert n == 2
    assert np.isclose(p, (2 / 3 + 1 / 3) / 2)
    assert np.isclose(r, (2 / 4 + 1 / 1) / 2)
    assert np.isclose(g, (dcg0 / idcg0 + 1.0) / 2)
    assert ref.ranking_metrics(ids[2:], rowptr[2:] - 5, colidx[5:], val[5:]) == (0, 0.0, 0.0, 0.0)
