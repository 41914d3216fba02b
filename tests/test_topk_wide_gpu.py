"""Top-k above k = 128 (cumf_topk_wide) on the GPU against the numpy reference of tests/topk_ref.py: ids and score bits exact
on dyadic data (where the reference is the exact fmaf chain, and equal scores are frequent) at the seams of the selection, in
every arrival order, across slabs, against cumf_topk up to k = 128, and through the engines."""
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


def _run(dev, Q, C, k, exclude=None, entry=None):
    """(ids, scores) as numpy of als.topk, or of the C entry point `entry` called directly."""
    import torch

    from cumf_als_amd import als

    q, c = torch.from_numpy(Q).to(dev), torch.from_numpy(C).to(dev)
    ex = None if exclude is None else tuple(torch.from_numpy(np.asarray(x, t)).to(dev) for x, t in zip(exclude, (np.int64, np.int32)))
    if entry is None:
        ids, sc = als.topk(q, c, k, ex)
    else:
        ids = torch.empty((len(Q), k), dtype=torch.int32, device=dev)
        sc = torch.empty((len(Q), k), dtype=torch.float32, device=dev)
        assert entry(q.data_ptr(), len(Q), c.data_ptr(), len(C), Q.shape[1], None, 0, None, k, ids.data_ptr(), sc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def _assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


def _csr(rng, rows, ncand):
    """Exclusion rows with duplicates, ascending; query 1 excludes every candidate."""
    cols = [np.sort(rng.randint(0, ncand, ncand // 8)) for _ in range(rows)]
    cols[1] = np.arange(ncand)
    return np.concatenate([[0], np.cumsum([len(c) for c in cols])]), np.concatenate(cols).astype(np.int32), cols


F, K, NCAND = (3, 100, 129), (129, 193, 1000, 2048), (-1, 0, 1, 65, None)  # ncand = k + d; None: 3 k + 7
SEAMS = [(F[(i + j) % 3], k, d, (i + j) % 2 == 1) for i, k in enumerate(K) for j, d in enumerate(NCAND)]
SEAMS += [(F[(j + 1) % 3], k, d, j % 2 == 0) for k in (193, 2048) for j, d in enumerate(NCAND)]


@pytest.mark.parametrize("f,k,d,excl", SEAMS)
def test_selection_seams(dev, f, k, d, excl):
    rng = np.random.RandomState(7 * k + f)
    rows, ncand = 33, 3 * k + 7 if d is None else k + d
    Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
    C[ncand // 2] = np.nan
    rowptr, colidx, cols = _csr(rng, rows, ncand) if excl else (None, None, None)
    got = _run(dev, Q, C, k, (rowptr, colidx) if excl else None)
    _assert_same(got, ref.topk(ref.chain_scores(Q, C), k, cols))
    assert not excl or np.all(got[0][1] == -1)


@pytest.mark.parametrize("order", ["increasing", "decreasing", "equal"])
def test_arrival_order(dev, order):
    """f = 1, scores in the order of the index: every candidate survives and the list shifts by a whole buffer per flush;
    nothing survives after the first k; the index alone decides."""
    c = np.arange(5000, dtype=np.float32)
    C = {"increasing": c, "decreasing": -c, "equal": np.ones_like(c)}[order].reshape(-1, 1)
    Q = np.array([[1.0], [2.0], [0.5]], np.float32)
    _assert_same(_run(dev, Q, C, 1000), ref.topk(ref.chain_scores(Q, C), 1000))


@pytest.mark.parametrize("k", [129, 2048])
@pytest.mark.parametrize("excl", [False, True])
def test_slabs_and_sub_range(dev, k, excl):
    """Five queries: several slabs; at k = 2048 every partial list is shorter than k.  A call on Q[2:] with offset row
    pointers returns rows 2.. of the full call."""
    rng = np.random.RandomState(k)
    rows, ncand, f = 5, 5000, 16
    Q, C = ref.dyadic(rng, (rows, f)), ref.dyadic(rng, (ncand, f))
    rowptr, colidx, cols = _csr(rng, rows, ncand) if excl else (None, None, None)
    full = _run(dev, Q, C, k, (rowptr, colidx) if excl else None)
    _assert_same(full, ref.topk(ref.chain_scores(Q, C), k, cols))
    _assert_same(_run(dev, Q[2:], C, k, (rowptr[2:], colidx) if excl else None), (full[0][2:], full[1][2:]))


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("f", [16, 130])
def test_agrees_with_the_narrow_path(dev, alslib, f, k):
    rng = np.random.RandomState(f + k)
    Q, C = rng.standard_normal((129, f)).astype(np.float32), rng.standard_normal((391, f)).astype(np.float32)
    wide = _run(dev, Q, C, k, entry=alslib.cumf_topk_wide)
    _assert_same(wide, _run(dev, Q, C, k))
    _assert_same(_run(dev, Q, C, k, entry=alslib.cumf_topk_wide), wide)


def test_engine_recommends_300(dev):
    from cumf_als_amd import als, datagen
    from tests.test_topk_gpu import _check_engine_topk  # recommend and ranking_metrics against the reference

    eng = als.ALSEngine(datagen.synth_ratings(300, 400, 12_000, 3_000, seed=3).to(dev), 32, 0.05)
    eng.init_factors(seed=1)
    eng.iterate(1)
    for side in ("x", "theta"):
        _check_engine_topk(eng, side, 300)
    eng.close()


def test_biased_engine_recommends_200(dev):
    """recommend(200) on 200 items: every unseen item of a row, best first, and mu + score is predict(u, id) bit for bit."""
    from cumf_als_amd import als, datagen
    from tests import bias_ref

    R, train, test = bias_ref.planted_bias_ratings()
    (tr, tc), (er, ec) = np.nonzero(train), np.nonzero(test)
    r = datagen.from_coo(*R.shape, tr, tc, R[train].astype(np.float32), er, ec, R[test].astype(np.float32)).to(dev)
    eng = als.BiasedALSEngine(r, 8, 0.05, solver="lu")
    eng.init_factors(bias_ref.theta0(r.n, 8).astype(np.float32))
    eng.iterate(2)
    ids, scores = (t.cpu().numpy() for t in eng.recommend(200))
    valid = ids >= 0
    assert np.array_equal(valid.sum(1), (~train).sum(1)) and not train[np.nonzero(valid)[0], ids[valid]].any()
    assert np.all(scores[:, :-1] >= scores[:, 1:]) and np.all(np.isneginf(scores[~valid]))
    pred = eng.predict(np.nonzero(valid)[0], ids[valid]).cpu().numpy()
    assert np.array_equal((np.float32(eng.mu) + scores[valid]).view(np.int32), pred.view(np.int32))
    eng.close()
