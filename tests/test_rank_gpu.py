"""Full-ranking evaluation on the GPU against the numpy reference of tests/rank_ref.py.  On dyadic data the reference scores
are exactly the fmaf chain, so ranks and n_eligible must EQUAL the reference: ties, exclusion, NaN, rows of any length, both
row-pointer widths, batching, determinism; then the ranks against cumf_topk's lists, the metrics, and both engines."""
import numpy as np
import pytest

from tests import rank_ref as ref
from tests import topk_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(alslib):
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _csr(rows_cols):
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_cols])]).astype(np.int64)
    colidx = (np.concatenate(rows_cols) if len(rows_cols) else np.zeros(0)).astype(np.int32)
    return rowptr, colidx


def _random_rows(rng, rows, ncand, mean, unique=True):
    out = []
    for n in rng.poisson(mean, rows):
        n = min(int(n), ncand)
        out.append(np.sort(rng.choice(ncand, n, replace=False) if unique else rng.randint(0, ncand, n)))
    return out


def _run(dev, Q, C, test, exclude=None, tdtype=np.int64, xdtype=np.int64):
    import torch

    from cumf_als_amd import als

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ex = None if exclude is None else (t(exclude[0].astype(xdtype)), t(exclude[1]))
    ranks, ne = als.heldout_ranks(t(Q), t(C), t(test[0].astype(tdtype)), t(test[1]), ex)
    torch.cuda.synchronize()
    return ranks.cpu().numpy(), ne.cpu().numpy()


def _check(dev, Q, C, test_rows, excl_rows=None, **kw):
    test = _csr(test_rows)
    s = topk_ref.chain_scores(Q, C)
    want = ref.heldout_ranks(s, test[0], test[1], excl_rows)
    got = _run(dev, Q, C, test, None if excl_rows is None else _csr(excl_rows), **kw)
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])
    return got


# few queries x many candidates (the candidates split into slabs) and many queries x few candidates (one slab)
@pytest.mark.parametrize("f", [1, 3, 16, 100, 129, 512])
@pytest.mark.parametrize("shape", ["few_queries", "many_queries"])
def test_ranks_exact_dyadic(dev, f, shape):
    rng = np.random.RandomState(f)
    rows, ncand = (8, 200_000 if f <= 100 else 40_000) if shape == "few_queries" else (1500 if f <= 100 else 400, 1000)
    Q, C = topk_ref.dyadic(rng, (rows, f)), topk_ref.dyadic(rng, (ncand, f))
    excl = _random_rows(rng, rows, ncand, 30, unique=False)
    _check(dev, Q, C, _random_rows(rng, rows, ncand, 12), excl)


def test_ranks_ties_duplicated_candidates(dev):
    rng = np.random.RandomState(21)
    Q, C = topk_ref.dyadic(rng, (200, 24)), topk_ref.dyadic(rng, (5000, 24))
    C[rng.choice(5000, 2000, replace=False)] = C[:20][rng.randint(0, 20, 2000)]
    _check(dev, Q, C, _random_rows(rng, 200, 5000, 40), _random_rows(rng, 200, 5000, 100, unique=False))


def test_ranks_all_zero_table(dev):
    rng = np.random.RandomState(22)
    rows, ncand = 70, 3000
    Q, C = topk_ref.dyadic(rng, (rows, 8)), np.zeros((ncand, 8), np.float32)
    test, excl = _random_rows(rng, rows, ncand, 20), _random_rows(rng, rows, ncand, 50, unique=False)
    ranks, ne = _check(dev, Q, C, test, excl)
    rowptr, colidx = _csr(test)
    for q in range(rows):  # every score ties: the rank is the index order minus the exclusions in front
        ex = np.unique(excl[q])
        for e in range(rowptr[q], rowptr[q + 1]):
            t = colidx[e]
            assert ranks[e] == (-1 if t in ex else t - np.searchsorted(ex, t))


def test_ranks_ties_across_slabs(dev):
    rng = np.random.RandomState(5)
    Q = rng.randint(-1, 2, (6, 8)).astype(np.float32)
    C = rng.randint(-1, 2, (150_000, 8)).astype(np.float32)
    _check(dev, Q, C, _random_rows(rng, 6, 150_000, 200))


def test_ranks_exclusion_and_out_of_table(dev):
    rng = np.random.RandomState(7)
    for rows, ncand, f in ((300, 2000, 32), (5, 60_000, 16)):
        Q, C = topk_ref.dyadic(rng, (rows, f)), topk_ref.dyadic(rng, (ncand, f))
        excl = _random_rows(rng, rows, ncand, ncand / 20, unique=False)  # duplicates in the exclusion rows
        excl[1] = np.arange(ncand)                                       # query 1 excludes every candidate
        test = _random_rows(rng, rows, ncand, 15)
        test[0] = np.unique(np.concatenate([test[0], excl[0][:5]]))      # held-out entries that are also excluded
        test[2] = np.concatenate([test[2], [ncand, ncand + 7, 2**31 - 1]])  # ... and outside the table
        ranks, ne = _check(dev, Q, C, test, excl)
        rowptr, colidx = _csr(test)
        assert ne[1] == 0 and np.all(ranks[rowptr[1]:rowptr[2]] == -1)
        assert np.all(ranks[rowptr[0]:rowptr[1]][np.isin(test[0], excl[0])] == -1)
        assert np.all(ranks[rowptr[3] - 3:rowptr[3]] == -1)


def test_ranks_nan(dev):
    rng = np.random.RandomState(11)
    Q, C = topk_ref.dyadic(rng, (200, 24)), topk_ref.dyadic(rng, (30_000, 24))
    nan_c = rng.choice(30_000, 500, replace=False)
    C[nan_c] = np.nan
    Q[[3, 150]] = np.nan
    test = _random_rows(rng, 200, 30_000, 10)
    test[5] = np.unique(np.concatenate([test[5], nan_c[:4]]))
    ranks, ne = _check(dev, Q, C, test)
    rowptr, colidx = _csr(test)
    assert ne[3] == 0 and ne[150] == 0 and ne[5] == 30_000 - 500
    assert np.all(ranks[rowptr[3]:rowptr[4]] == -1) and np.all(ranks[rowptr[150]:rowptr[151]] == -1)
    assert np.all(ranks[rowptr[5]:rowptr[6]][np.isin(test[5], nan_c)] == -1)


def test_ranks_rows_of_every_length(dev):
    rng = np.random.RandomState(23)
    rows, ncand, f = 140, 9000, 20
    Q, C = topk_ref.dyadic(rng, (rows, f)), topk_ref.dyadic(rng, (ncand, f))
    test = _random_rows(rng, rows, ncand, 5)
    for q, n in ((0, 0), (1, 1), (2, 33), (3, 5500), (64, 8000), (65, 0), (139, 700)):
        test[q] = np.sort(rng.choice(ncand, n, replace=False))
    _check(dev, Q, C, test, _random_rows(rng, rows, ncand, 300, unique=False))


@pytest.mark.parametrize("tdtype", [np.int32, np.int64])
@pytest.mark.parametrize("xdtype", [np.int32, np.int64])
def test_ranks_row_pointer_widths(dev, tdtype, xdtype):
    rng = np.random.RandomState(29)
    Q, C = topk_ref.dyadic(rng, (150, 16)), topk_ref.dyadic(rng, (4000, 16))
    _check(dev, Q, C, _random_rows(rng, 150, 4000, 8), _random_rows(rng, 150, 4000, 60, unique=False), tdtype=tdtype,
           xdtype=xdtype)


def test_ranks_batching_and_determinism(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(13)
    rows, ncand, f = 700, 20_000, 100
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    Q, C = t(rng.standard_normal((rows, f)).astype(np.float32)), t(rng.standard_normal((ncand, f)).astype(np.float32))
    xr, xc = _csr(_random_rows(rng, rows, ncand, 100, unique=False))
    tr, tc = _csr(_random_rows(rng, rows, ncand, 10))
    ex, tr, tc = (t(xr.astype(np.int32)), t(xc)), t(tr), t(tc)
    full = [x.cpu().numpy() for x in als.heldout_ranks(Q, C, tr, tc, ex)]
    again = [x.cpu().numpy() for x in als.heldout_ranks(Q, C, tr, tc, ex)]
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
    ranks = torch.full_like(tc, -7)
    ne = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    for a, b in ((0, 129), (129, 391), (391, rows)):  # Q, the row pointers and n_eligible offset; ranks keeps its base
        als.heldout_ranks(Q[a:b], C, tr[a:b + 1], tc, (ex[0][a:b + 1], ex[1]), out=(ranks, ne[a:b]))
    assert np.array_equal(ranks.cpu().numpy(), full[0]) and np.array_equal(ne.cpu().numpy(), full[1])


def test_ranks_against_topk_lists(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(31)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    for rows, ncand, f in ((300, 5000, 100), (6, 70_000, 64)):  # trained-like factors: both sides compute the same bits
        Q, C = t((0.3 * rng.standard_normal((rows, f))).astype(np.float32)), t((0.3 * rng.standard_normal((ncand, f))).astype(np.float32))
        excl = _random_rows(rng, rows, ncand, 50, unique=False)
        test = _random_rows(rng, rows, ncand, 600)
        xr, xc = _csr(excl)
        tr, tc = _csr(test)
        ex = (t(xr), t(xc))
        ids = als.topk(Q, C, 128, ex)[0].cpu().numpy()
        ranks = als.heldout_ranks(Q, C, t(tr), t(tc), ex)[0].cpu().numpy()
        hits = 0
        for q in range(rows):
            pos = {int(c): j for j, c in enumerate(ids[q]) if c >= 0}
            for e in range(tr[q], tr[q + 1]):
                j = pos.get(int(tc[e]))
                assert (j is not None) == (0 <= ranks[e] < 128), (q, e)
                if j is not None:
                    assert ranks[e] == j, (q, e)
                    hits += 1
        assert hits > 0  # the lists and the held-out rows do overlap


def _assert_metrics(got, want, tol=1e-12):
    assert got["queries"] == want["queries"] and got["auc_queries"] == want["auc_queries"]
    for key in ("auc", "mpr", "mrr", "map"):
        assert abs(got[key] - want[key]) <= tol * abs(want[key]), (key, got[key], want[key])
    for key in ("precision", "recall", "ndcg"):
        assert list(got[key]) == list(want[key])
        for k in want[key]:
            assert abs(got[key][k] - want[key][k]) <= tol * abs(want[key][k]), (key, k, got[key][k], want[key][k])


def test_rank_metrics_matches_reference(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(17)
    rows, ncand = 500, 3000
    lens = rng.randint(0, 60, rows)
    lens[:3] = 0
    lens[7] = 2500  # a row the wave sorts in many passes
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ranks = np.concatenate([rng.choice(ncand, n, replace=False) for n in lens]).astype(np.int32)  # distinct within a row
    ranks[rng.random_sample(len(ranks)) < 0.1] = -1
    ne = np.full(rows, ncand, np.int32)
    ne[10], ne[11], ne[12] = 1, 0, lens[12]  # N <= 1 (no MPR term) and N == p at most (no AUC term)
    ranks[rowptr[10]:rowptr[11]] = -1
    ranks[rowptr[10]:rowptr[11]][:1] = 0
    ranks[rowptr[11]:rowptr[12]] = -1
    ranks[rowptr[12]:rowptr[13]] = np.arange(lens[12])
    val = rng.choice([-1.0, 0.0, 1.0, 4.0], len(ranks)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    ks = (1, 128, 1000, ncand + 5)
    for v in (None, val):
        for rp in (rowptr, rowptr.astype(np.int32)):
            got = als.rank_metrics(t(ranks), t(ne), t(rp), None if v is None else t(v), ks)
            _assert_metrics(got, ref.rank_metrics(ranks, ne, rowptr, v, ks))
    empty = als.rank_metrics(t(np.full(4, -1, np.int32)), t(np.zeros(2, np.int32)), t(np.array([0, 1, 4])), None, (10,))
    assert empty == {"queries": 0, "auc_queries": 0, "auc": 0.0, "mpr": 0.0, "mrr": 0.0, "map": 0.0, "precision": {10: 0.0},
                     "recall": {10: 0.0}, "ndcg": {10: 0.0}}


def test_rank_metrics_of_device_ranks(dev):
    import torch

    from cumf_als_amd import als

    rng = np.random.RandomState(19)
    rows, ncand, f = 260, 2500, 16
    Q, C = topk_ref.dyadic(rng, (rows, f)), topk_ref.dyadic(rng, (ncand, f))
    test, excl = _random_rows(rng, rows, ncand, 30), _random_rows(rng, rows, ncand, 200, unique=False)
    tr, tc = _csr(test)
    xr, xc = _csr(excl)
    val = rng.choice([-1.0, 1.0, 2.5], len(tc)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    ranks, ne = als.heldout_ranks(t(Q), t(C), t(tr), t(tc), (t(xr), t(xc)))
    want = ref.heldout_ranks(topk_ref.chain_scores(Q, C), tr, tc, excl)
    ks = (1, 10, 128, 1000, 5000)
    _assert_metrics(als.rank_metrics(ranks, ne, t(tr), t(val), ks), ref.rank_metrics(want[0], want[1], tr, val, ks))


def test_engines_full_ranking_metrics(dev):
    import torch

    from cumf_als_amd import als, datagen

    r = datagen.synth_ratings(300, 400, 12_000, 3_000, seed=3)
    # a held-out set disjoint from training: the two definitions of |T_u| differ only on train n test
    d = r.numpy()
    train = set(zip(np.repeat(np.arange(r.m), np.diff(d["csr_indptr"])).tolist(), d["csr_indices"].tolist()))
    keep = np.array([(int(a), int(b)) not in train for a, b in zip(d["test_row"], d["test_col"])])
    first = np.zeros(len(keep), bool)
    first[np.unique(d["test_row"].astype(np.int64) * r.n + d["test_col"], return_index=True)[1]] = True
    keep &= first  # and unique within each row, as the held-out CSR must be
    assert keep.sum() > 1000
    r = r.to(dev)
    sel = torch.from_numpy(np.nonzero(keep)[0]).to(dev)
    r.test_row, r.test_col, r.test_data = r.test_row[sel], r.test_col[sel], r.test_data[sel]
    for make, side in ((lambda: als.ImplicitALSEngine(r, 32, 0.05, 2.0), "x"), (lambda: als.ALSEngine(r, 32, 0.05), "theta")):
        eng = make()
        eng.init_factors(seed=1)
        eng.iterate(2)
        old = eng.ranking_metrics(10, side)
        new = eng.full_ranking_metrics(side, ks=(10,))
        assert new["queries"] == old["queries"] > 0
        for key in ("precision", "recall", "ndcg"):
            assert abs(new[key][10] - old[key]) <= 1e-12, (key, new[key][10], old[key])
        assert 0.0 <= new["mpr"] <= 1.0 and 0.0 <= new["auc"] <= 1.0 and 0.0 < new["mrr"] <= 1.0
        ranks, ne, rowptr, colidx = eng.heldout_ranks(side)
        assert ranks.shape == colidx.shape and int(ranks.min()) >= 0 and ne.shape[0] == rowptr.shape[0] - 1
        eng.close()
