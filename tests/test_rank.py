"""Full-ranking evaluation without a GPU: the C ABI of include/cumf_rank_capi.h is exported and listed, its scope check, and
self-checks of the numpy reference that tests/test_rank_gpu.py measures against."""
import os
import re

import numpy as np

from tests import rank_ref as ref
from tests import topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_header_symbols_are_exported(alslib):
    from cumf_als_amd import lib

    text = open(os.path.join(ROOT, "include", "cumf_rank_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cumf_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared and set(declared) == set(lib.RANK_SYMBOLS), (declared, lib.RANK_SYMBOLS)
    for s in declared:
        assert hasattr(alslib, s), s


def test_rank_available_table(alslib):
    for f in (0, 1, 512, 513):
        assert alslib.cumf_rank_available(f) == int(1 <= f <= 512), f


def test_reference_ranks_hand_computed():
    # candidates 0..6; order of the eligible ones by (score desc, index asc): 1, 3, 6, 5, 0, 4 (2 is NaN)
    s = np.array([[1.0, 3.0, np.nan, 3.0, -np.inf, 2.0, 3.0], [0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    rowptr = np.array([0, 5, 5, 8])  # row 1 of the CSR below is empty; three rows against two score rows: use rows 0, 0, 1
    s3 = s[[0, 0, 1]]
    colidx = np.array([0, 2, 3, 6, 9, 1, 4, 6])
    ranks, ne = ref.heldout_ranks(s3, rowptr, colidx)
    assert ranks.tolist() == [4, -1, 1, 2, -1, 1, 4, 6]  # NaN and out of the table: -1; -0 ties with +0: index order
    assert ne.tolist() == [6, 6, 7]
    # excluding 3 (twice) and 5 moves 6 up to rank 1 and 0 to rank 2; an excluded held-out entry gets -1
    ranks, ne = ref.heldout_ranks(s3, rowptr, colidx, exclude=[[3, 3, 5], [], [0, 1, 2, 3]])
    assert ranks.tolist() == [2, -1, -1, 1, -1, -1, 0, 2]
    assert ne.tolist() == [4, 6, 3]


def _case(seed, rows=40, ncand=300, f=12, mean_test=6, with_excl=True):
    rng = np.random.RandomState(seed)
    Q, C = topk_ref.dyadic(rng, (rows, f)), topk_ref.dyadic(rng, (ncand, f))
    C[rng.choice(ncand, 10, replace=False)] = C[0]  # ties
    s = topk_ref.chain_scores(Q, C)
    excl = [np.sort(rng.choice(ncand, rng.randint(0, 40), replace=False)) for _ in range(rows)] if with_excl else None
    test = []
    for q in range(rows):
        pool = np.setdiff1d(np.arange(ncand), excl[q]) if with_excl else np.arange(ncand)
        test.append(np.sort(rng.choice(pool, min(len(pool), rng.poisson(mean_test)), replace=False)))
    rowptr = np.concatenate([[0], np.cumsum([len(t) for t in test])])
    colidx = np.concatenate(test).astype(np.int32)
    return s, excl, rowptr, colidx, rng


def test_reference_rank_is_position_in_topk():
    s, excl, rowptr, colidx, _ = _case(1)
    ranks, ne = ref.heldout_ranks(s, rowptr, colidx, excl)
    for k in (1, 10, 128):
        ids, _ = topk_ref.topk(s, k, excl)
        for q in range(s.shape[0]):
            for e in range(rowptr[q], rowptr[q + 1]):
                pos = np.nonzero(ids[q] == colidx[e])[0]
                assert (ranks[e] < k) == (len(pos) == 1)
                if len(pos):
                    assert ranks[e] == pos[0]
    assert np.array_equal(ne, [s.shape[1] - len(x) for x in excl])


def test_reference_auc_is_pair_counting():
    s, excl, rowptr, colidx, rng = _case(2, rows=12, ncand=80)
    val = rng.choice([-1.0, 1.0, 3.0], len(colidx)).astype(np.float32)
    ranks, ne = ref.heldout_ranks(s, rowptr, colidx, excl)
    for v in (None, val):
        total, n = 0.0, 0
        for q in range(s.shape[0]):
            ent = np.arange(rowptr[q], rowptr[q + 1])
            pos = [int(colidx[e]) for e in ent if v is None or v[e] > 0]
            elig = [c for c in range(s.shape[1]) if c not in set(excl[q].tolist()) and not np.isnan(s[q, c])]
            neg = [c for c in elig if c not in pos]
            if not pos or not neg:
                continue
            before = lambda a, b: s[q, a] > s[q, b] or (s[q, a] == s[q, b] and a < b)  # noqa: E731
            total += sum(before(a, b) for a in pos for b in neg) / (len(pos) * len(neg))
            n += 1
        got = ref.rank_metrics(ranks, ne, rowptr, v)
        assert got["auc_queries"] == n
        assert abs(got["auc"] - total / n) <= 1e-12


def test_reference_cutoff_metrics_match_topk_metrics():
    s, excl, rowptr, colidx, rng = _case(3)  # held-out sets disjoint from the exclusion
    val = rng.choice([-1.0, 0.0, 1.0, 4.0], len(colidx)).astype(np.float32)
    ranks, ne = ref.heldout_ranks(s, rowptr, colidx, excl)
    for v in (None, val):
        got = ref.rank_metrics(ranks, ne, rowptr, v, ks=(1, 10, 128))
        for k in (1, 10, 128):
            ids, _ = topk_ref.topk(s, k, excl)
            n, p, r, g = topk_ref.ranking_metrics(ids, rowptr, colidx, v)
            assert got["queries"] == n
            assert abs(got["precision"][k] - p) <= 1e-12 and abs(got["recall"][k] - r) <= 1e-12
            assert abs(got["ndcg"][k] - g) <= 1e-12


def test_reference_mpr_mrr_map_hand_computed():
    # query 0: N = 11, relevant ranks (0, 4) with weights (2, 1) and one entry without a rank; query 1: nothing relevant
    ranks = np.array([4, -1, 0, 7], np.int32)
    rowptr = np.array([0, 3, 4])
    val = np.array([1.0, 5.0, 2.0, 0.0], np.float32)
    got = ref.rank_metrics(ranks, np.array([11, 20]), rowptr, val, ks=(3,))
    assert got["queries"] == 1 and got["auc_queries"] == 1
    assert np.isclose(got["mpr"], (2 * 0 / 10 + 1 * 4 / 10) / 3)
    assert np.isclose(got["mrr"], 1.0)
    assert np.isclose(got["map"], (1 / 1 + 2 / 5) / 2)
    assert np.isclose(got["auc"], 1 - ((0 - 0) + (4 - 1)) / (2 * 9))
    assert np.isclose(got["precision"][3], 1 / 3) and np.isclose(got["recall"][3], 1 / 2)
    assert np.isclose(got["ndcg"][3], 1.0 / (1.0 + 1 / np.log2(3)))
