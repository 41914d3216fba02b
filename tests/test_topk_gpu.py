"""Top-k recommendation and ranking metrics on the GPU against the numpy reference of tests/topk_ref.py: bit-exact ids and
scores on dyadic data (where the reference is the exact fmaf chain), exclusion, NaN, batching, determinism, the metrics,
and both engines' recommend / ranking_metrics."""
import numpy as np
import pytest

from tests import topk_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(alslib):
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _run(dev, Q, C, k, exclude=None):
    import torch

    from cumf_als_amd import als

    ex = None
    if exclude is not None:
        ex = (torch.from_numpy(np.asarray(exclude[0], np.int64)).to(dev), torch.from_numpy(np.asarray(exclude[1], np.int32)).to(dev))
    ids, sc = als.topk(torch.from_numpy(Q).to(dev), torch.from_numpy(C).to(dev), k, ex)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def _assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


# few queries x many candidates (slabs + the merge kernel) and many queries x few candidates (one slab)
@pytest.mark.parametrize("f", [1, 3, 16, 100, 129, 512])
@pytest.mark.parametrize("shape", ["few_queries", "many_queries"])
def test_topk_exact_dyadic(dev, f, shape):
    rng = np.random.RandomState(f)
    rows, ncand = (8, 200_000 if f <= 100 else 40_000) if shape == "few_queries" else (1500 if f <= 100 else 400, 1000)
    Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
    s = ref.chain_scores(Q, C)
    for k in (1, 10, 128):
        _assert_same(_run(dev, Q, C, k), ref.topk(s, k))


def test_topk_ties_across_slabs(dev):
    rng = np.random.RandomState(5)
    Q = rng.randint(-1, 2, (6, 8)).astype(np.float32)
    C = rng.randint(-1, 2, (150_000, 8)).astype(np.float32)
    s = ref.chain_scores(Q, C)
    for k in (10, 128):
        _assert_same(_run(dev, Q, C, k), ref.topk(s, k))


def _random_csr(rng, rows, ncand, mean):
    lens = rng.poisson(mean, rows)
    cols = [np.sort(rng.randint(0, ncand, n)) for n in lens]  # duplicates allowed
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    return rowptr, np.concatenate(cols).astype(np.int32) if rows else np.zeros(0, np.int32)


def test_topk_exclusion(dev):
    rng = np.random.RandomState(7)
    for rows, ncand, f in ((300, 2000, 32), (5, 60_000, 16)):
        Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
        rowptr, colidx = _random_csr(rng, rows, ncand, ncand / 20)
        # query 1 excludes every candidate; query 2 leaves fewer than k eligible
        rows_cols = ref.csr_rows(rowptr, colidx)
        rows_cols[1] = np.arange(ncand, dtype=np.int32)
        keep = np.sort(rng.choice(ncand, 7, replace=False))
        rows_cols[2] = np.setdiff1d(np.arange(ncand), keep).astype(np.int32)
        rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_cols])])
        colidx = np.concatenate(rows_cols).astype(np.int32)
        s = ref.chain_scores(Q, C)
        for k in (10, 128):
            got = _run(dev, Q, C, k, (rowptr, colidx))
            _assert_same(got, ref.topk(s, k, rows_cols))
            assert np.all(got[0][1] == -1)
            assert np.array_equal(got[0][2, :7], keep[np.lexsort((keep, -s[2, keep].astype(np.float64)))])
            for q in range(rows):
                assert not np.isin(got[0][q], rows_cols[q]).any()


def test_topk_nan_rows(dev):
    rng = np.random.RandomState(11)
    Q, C = ref.dyadic(rng, (200, 24)), ref.dyadic(rng, (30_000, 24))
    C[rng.choice(30_000, 500, replace=False)] = np.nan
    Q[[3, 150]] = np.nan
    s = ref.chain_scores(Q, C)
    got = _run(dev, Q, C, 64)
    _assert_same(got, ref.topk(s, 64))
    assert np.all(got[0][3] == -1) and np.all(np.isneginf(got[1][150]))


def test_topk_batching_and_determinism(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(13)
    rows, ncand, f, k = 700, 20_000, 100, 50
    Q = torch.from_numpy(rng.standard_normal((rows, f)).astype(np.float32)).to(dev)
    C = torch.from_numpy(rng.standard_normal((ncand, f)).astype(np.float32)).to(dev)
    rowptr, colidx = _random_csr(rng, rows, ncand, 100)
    ex = (torch.from_numpy(rowptr.astype(np.int32)).to(dev), torch.from_numpy(colidx).to(dev))
    full = [t.cpu().numpy() for t in als.topk(Q, C, k, ex)]
    again = [t.cpu().numpy() for t in als.topk(Q, C, k, ex)]
    _assert_same(again, full)
    a, b = 129, 391
    part = [t.cpu().numpy() for t in als.topk(Q[a:b], C, k, (ex[0][a:b + 1], ex[1]))]
    _assert_same(part, (full[0][a:b], full[1][a:b]))


def test_ranking_metrics_matches_reference(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(17)
    rows, ncand, k = 500, 300, 20
    ids = np.stack([rng.choice(ncand, k, replace=False) for _ in range(rows)]).astype(np.int32)
    ids[rng.random_sample(ids.shape) < 0.1] = -1
    lens = rng.randint(0, 60, rows)  # |T_u| = 0 and |T_u| > k both occur
    lens[:3] = 0
    cols = [np.sort(rng.choice(ncand, n, replace=False)) for n in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    colidx = np.concatenate(cols).astype(np.int32)
    val = rng.choice([-1.0, 0.0, 1.0, 4.0], len(colidx)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    for v in (None, val):
        got = als.ranking_metrics(t(ids), t(rowptr.astype(np.int64)), t(colidx), None if v is None else t(v))
        n, p, r, g = ref.ranking_metrics(ids, rowptr, colidx, v)
        assert got["queries"] == n
        for key, want in (("precision", p), ("recall", r), ("ndcg", g)):
            assert abs(got[key] - want) <= 1e-12, (key, got[key], want)


def _check_engine_topk(eng, side, k):
    query, cand, seen, (trow, tcol, rows) = eng._side(side)
    ids, sc = (x.cpu().numpy() for x in eng.recommend(k, side))
    s = ref.chain_scores(query.cpu().numpy(), cand.cpu().numpy())
    wids, wsc = ref.topk(s, k, ref.csr_rows(seen[0].cpu().numpy(), seen[1].cpu().numpy()))
    # fp64-emulated fmaf can differ in the last bit on non-dyadic data: compare scores to 1 ulp-ish, ids where separated
    assert np.allclose(sc, wsc, rtol=1e-6, atol=1e-6)
    for q in range(ids.shape[0]):
        for j in range(k):
            close = [abs(float(wsc[q, j]) - float(wsc[q, i])) <= 1e-5 * max(1.0, abs(float(wsc[q, j])))
                     for i in (j - 1, j + 1) if 0 <= i < k]
            if not any(close):
                assert ids[q, j] == wids[q, j], (q, j)
    got = eng.ranking_metrics(k, side)
    row, col, val = trow.cpu().numpy(), tcol.cpu().numpy(), eng.r.test_data.cpu().numpy()
    order = np.lexsort((col, row))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))])
    n, p, r, g = ref.ranking_metrics(ids, rowptr, col[order], val[order])
    assert got["queries"] == n
    assert abs(got["precision"] - p) <= 1e-12 and abs(got["recall"] - r) <= 1e-12 and abs(got["ndcg"] - g) <= 1e-12


def test_engines_recommend_and_metrics(dev):
    from cumf_als_amd import als, datagen

    r = datagen.synth_ratings(300, 400, 12_000, 3_000, seed=3).to(dev)
    eng = als.ImplicitALSEngine(r, 32, 0.05, 2.0)
    eng.init_factors(seed=1)
    eng.iterate(2)
    _check_engine_topk(eng, "x", 10)
    eng.close()
    eng = als.ALSEngine(r, 32, 0.05)
    eng.init_factors(seed=1)
    eng.iterate(2)
    _check_engine_topk(eng, "theta", 10)
    eng.close()
