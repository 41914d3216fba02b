"""The seams of the scoring core that top-k and full ranking share (csrc/als_score.h): every case runs als.topk and
als.heldout_ranks on the same dyadic inputs and compares both bit for bit with tests/topk_ref.py / tests/rank_ref.py --
exclusions on the first and last candidate of every LDS block and slab, query counts around the wave and workgroup sizes
with candidate counts around one block -- and the column sum of the two metric reductions at empty, full and ragged strides."""
import numpy as np
import pytest

from tests import rank_ref
from tests import topk_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(alslib):
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _csr(rows_cols):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_cols])]).astype(np.int64)
    return rowptr, np.concatenate(rows_cols).astype(np.int32)


def _check_both(dev, Q, C, excl_rows, test_rows, ks):
    """top-k at every k of ks and the held-out ranks of one input, each EQUAL to its reference."""
    import torch

    from cumf_als_amd import als

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    s = ref.chain_scores(Q, C)
    ex = tuple(t(a) for a in _csr(excl_rows))
    for k in ks:
        ids, sc = (x.cpu().numpy() for x in als.topk(t(Q), t(C), k, ex))
        wids, wsc = ref.topk(s, k, excl_rows)
        assert np.array_equal(ids, wids), k
        assert np.array_equal(sc.view(np.int32), wsc.view(np.int32)), k
    tr, tc = _csr(test_rows)
    ranks, ne = (x.cpu().numpy() for x in als.heldout_ranks(t(Q), t(C), t(tr), t(tc), ex))
    wranks, wne = rank_ref.heldout_ranks(s, tr, tc, excl_rows)
    assert np.array_equal(ne, wne)
    assert np.array_equal(ranks, wranks)
    return ranks, ne


# Every query excludes the candidates 0 and 63 (mod 64): slab_len is a multiple of the 64-candidate block, so these are the
# first and last candidate of every block and of every slab, whatever the cut.  Query 0 lists each of them twice.
@pytest.mark.parametrize("rows,ncand", [(6, 150_000), (300, 1000)])  # several slabs + the merge kernel; one slab
def test_exclusion_at_block_and_slab_edges(dev, rows, ncand):
    rng = np.random.RandomState(rows)
    f = 16
    Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
    edge = np.nonzero(np.isin(np.arange(ncand) % 64, (0, 63)))[0]
    excl = [np.repeat(edge, 2) if q == 0 else edge for q in range(rows)]
    # held out: excluded edge candidates, their eligible neighbours (1 and 62 mod 64) and random ones
    test = []
    for q in range(rows):
        near = rng.choice(edge, 6)
        test.append(np.unique(np.concatenate([rng.choice(edge, 6), np.where(near % 64 == 0, near + 1, near - 1),
                                              rng.choice(ncand, 12)])))
    ranks, ne = _check_both(dev, Q, C, excl, test, (10, 128))
    assert np.all(ne == ncand - len(edge))
    tr, tc = _csr(test)
    assert np.array_equal(ranks == -1, np.isin(tc % 64, (0, 63)))


# rows around the 32 queries of a wave and the 128 of a workgroup, ncand around one block; f = 20: one feature chunk with a
# ragged group of 16, f = 132: two chunks, the second ragged
@pytest.mark.parametrize("f", [20, 132])
@pytest.mark.parametrize("rows", [31, 32, 33, 127, 128, 129])
def test_query_count_edges(dev, f, rows):
    for ncand in (63, 64, 65):
        rng = np.random.RandomState(1000 * f + 10 * rows + ncand)
        Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
        excl = [np.sort(rng.randint(0, ncand, rng.randint(0, 9))) for _ in range(rows)]
        test = [np.sort(rng.choice(ncand, rng.randint(0, 7), replace=False)) for _ in range(rows)]
        test[rows - 1] = np.array([0, ncand - 1])  # the last query, the first and last candidate
        _check_both(dev, Q, C, excl, test, (10, 128))


# rows: one stride with a single query, one short of full, full, one over, and several ragged strides of the 256 threads
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_metrics_reduce_strides(dev, rows):
    import torch

    from cumf_als_amd import als
    from tests.test_rank_gpu import _assert_metrics

    rng = np.random.RandomState(rows)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    ncand, k = 300, 20
    lens = rng.randint(1, 40, rows)
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    colidx = np.concatenate([np.sort(rng.choice(ncand, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.choice([-1.0, 0.0, 1.0, 4.0], len(colidx)).astype(np.float32)
    ids = np.stack([rng.choice(ncand, k, replace=False) for _ in range(rows)]).astype(np.int32)
    ranks = np.concatenate([rng.choice(ncand, n, replace=False) for n in lens]).astype(np.int32)  # distinct within a row
    ranks[rng.random_sample(len(ranks)) < 0.1] = -1
    ne = np.full(rows, ncand, np.int32)
    ks = (1, 10, 128)
    for v in (None, val):
        got = als.ranking_metrics(t(ids), t(rowptr), t(colidx), None if v is None else t(v))
        n, p, r, g = ref.ranking_metrics(ids, rowptr, colidx, v)
        assert got["queries"] == n
        for key, want in (("precision", p), ("recall", r), ("ndcg", g)):
            assert abs(got[key] - want) <= 1e-12, (key, got[key], want)  # (test_ranking_metrics_matches_reference's bound)
        _assert_metrics(als.rank_metrics(t(ranks), t(ne), t(rowptr), None if v is None else t(v), ks),
                        rank_ref.rank_metrics(ranks, ne, rowptr, v, ks))  # (test_rank_metrics_matches_reference's bound)
