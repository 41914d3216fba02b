"""The weighted block solver (als.update_weighted_block, WeightedALSEngine(solver="block")) on the MI355X: the fused kernels
(with and without the Gram term) and the segmented route against the block Gauss-Seidel recurrence in numpy on the dense
fp64 systems of tests/weighted_ref.py and tests/weighted_rank1_ref.py; the recurrence in float32 is the error scale."""
import functools

import numpy as np
import pytest
import torch

from tests import weighted_rank1_ref as ref1
from tests import weighted_ref as ref

pytestmark = pytest.mark.gpu

LAM, W0 = 0.05, 0.25
# tests/test_block_explicit_gpu.py's rows: the MFMA K tail, the groups in flight, the opening pass's reductions, the 64-entry
# load, the capacity classes (960 and 2048 here too), the fused / segmented seam and three segments
LENS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 128, 959, 960, 961, 2047, 2048, 2049, 4097]
N_COLS = 4200
ZERO_ROW = LENS.index(17)  # a live row whose weights are all 0
MODES = ("w0=0", "scalar", "rank1")


def block_ref(A, b, x0, sweeps, lens, B=32):
    """`sweeps` sweeps of exact block Gauss-Seidel on A x = b from x0, in the dtype of A; rows without entries get 0."""
    x = x0.astype(A.dtype)
    for u in np.flatnonzero(np.asarray(lens) > 0):
        for c in [c for _ in range(sweeps) for c in range(0, x.shape[1], B)]:
            x[u, c:c + B] += np.linalg.solve(A[u, c:c + B, c:c + B], (b[u] - A[u] @ x[u])[c:c + B])
    x[np.asarray(lens) == 0] = 0
    return x


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _systems(c, mode, Y, reg, dtype, csr=None):
    rowptr, colidx, val, wgt = csr or (c["rowptr"], c["colidx"], c["val"], c["wgt"])
    if mode == "rank1":
        return ref1.systems(rowptr, colidx, val, wgt, Y, LAM, c["own"], c["gat"], reg, dtype)
    return ref.systems(rowptr, colidx, val, wgt, Y, LAM, W0 if mode == "scalar" else 0.0, reg, dtype)


@functools.lru_cache(maxsize=4)
def _case(f, mode, reg="weighted"):
    rng = np.random.RandomState(7)
    c = {"rowptr": np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)}
    c["colidx"] = np.concatenate([np.sort(rng.choice(N_COLS, ln, replace=False)) for ln in LENS]).astype(np.int32)
    nnz = int(c["rowptr"][-1])
    c["val"] = rng.choice(np.array([0.5, 1.0, 2.0, 3.0, 4.0, 5.0], np.float32), nnz)
    c["wgt"] = rng.choice(np.array([0, 0.25, 0.5, 1.0, 2.0, 4.0], np.float32), nnz)
    c["wgt"][c["rowptr"][ZERO_ROW]:c["rowptr"][ZERO_ROW + 1]] = 0
    c["own"] = (rng.uniform(0.1, 0.5, len(LENS)) * (rng.rand(len(LENS)) > 0.1)).astype(np.float32)
    gat = (rng.uniform(0.05, 1.0, N_COLS) * (rng.rand(N_COLS) > 0.1)).astype(np.float32)
    c["gat"] = (gat / gat.max()).astype(np.float32)  # the largest gather weight is exactly 1
    c["Y"] = (0.3 * np.random.RandomState(3).standard_normal((N_COLS, f))).astype(np.float32)
    c["x0"] = (0.05 * np.random.RandomState(9).standard_normal((len(LENS), f))).astype(np.float32)
    c["sys"] = {d: _systems(c, mode, c["Y"], reg, d) for d in (np.float64, np.float32)}
    return c


def _update(c, mode, f, sweeps, route="auto", cuts=None, chunk=0, reg="weighted", w0=None):
    from cumf_als_amd import als

    Yg, x = _dev(c["Y"]), _dev(c["x0"].copy())
    w0 = (W0 if mode == "scalar" else 0.0) if w0 is None else w0
    unobserved = (_dev(c["own"]), _dev(c["gat"])) if mode == "rank1" else None
    G = als.weighted_gram(Yg, unobserved[1]) if unobserved else als.implicit_gram(Yg) if w0 > 0 else None
    cuts = cuts or [0, len(LENS)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        plan = als.Plan(c["rowptr"], f, lo, hi, chunk)
        als.update_weighted_block(plan, _dev(c["colidx"]), _dev(c["val"]), _dev(c["wgt"]), Yg, G, x, LAM, w0, reg, sweeps, route,
                                  unobserved)
        torch.cuda.synchronize()
        # the fused launches come last; a plan without a row of at most 2048 entries has none
        fused = route == "auto" and min(LENS[lo:hi]) <= 2048
        want = (("block_fused_gram_kernel", "block_row_kernel") if G is not None else
                ("block_fused_kernel", "block_row_free_kernel"))[0 if fused else 1]
        assert want in als.last_kernel_name(), (want, als.last_kernel_name())
        plan.close()
    return x.cpu().numpy()


def _stats(v):
    return float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max())


def _check(tag, x, x64, x32, live, c=2.0):
    """Per row the max-norm distance to the fp64 reference; its median / q90 / max over the live rows within c x those of the
    float32 reference + 1e-5 of the factors' scale (the bound form of tests/test_block_explicit_gpu.py)."""
    assert (x[~live] == 0).all(), tag
    scale = np.abs(x64).max()
    e_h, e_o = np.abs(x - x64).max(1)[live], np.abs(x32 - x64).max(1)[live]
    print(f"weighted block {tag}: hip {_stats(e_h)} numpy32 {_stats(e_o)} ratios "
          f"{[round(h / o, 3) for h, o in zip(_stats(e_h), _stats(e_o))]}")
    for sh, so in zip(_stats(e_h), _stats(e_o)):
        assert sh <= c * so + 1e-5 * scale, (tag, _stats(e_h), _stats(e_o))


PARITY = [(f, route, "weighted") for f in (8, 34, 66, 130, 510) for route in ("auto", "segmented")
          if route == "auto" or f in (34, 510)] + [(66, "auto", "plain")]


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("f,route,reg", PARITY)
def test_weighted_block_step_parity(alslib, mode, f, route, reg, sweeps):
    c = _case(f, mode, reg)
    # two plans: the rows of at most 2048 entries (the fused kernel alone under "auto") and the longer ones
    x = _update(c, mode, f, sweeps, route, cuts=[0, LENS.index(2049), len(LENS)], reg=reg)
    (A64, b64), (A32, b32) = c["sys"][np.float64], c["sys"][np.float32]
    _check(f"{mode} f={f} sweeps={sweeps} {route} {reg}", x, block_ref(A64, b64, c["x0"], sweeps, LENS),
           block_ref(A32, b32, c["x0"], sweeps, LENS), np.asarray(LENS) > 0)


@pytest.mark.parametrize("f", [8, 32])
def test_one_sweep_is_the_exact_solve(alslib, f):
    c = _case(f, "scalar")
    x = _update(c, "scalar", f, 1)
    live = np.asarray(LENS) > 0
    sol = {}
    for d, (A, b) in c["sys"].items():
        sol[d] = np.zeros_like(b)
        sol[d][live] = np.linalg.solve(A[live], b[live][..., None])[..., 0]
    _check(f"exact f={f}", x, sol[np.float64], sol[np.float32], live)


def test_weighted_block_reductions(alslib):
    """The special cases and the plan's cuts, bit for bit."""
    from cumf_als_amd import als

    f, rows = 66, len(LENS)
    c = _case(f, "scalar")
    ones = dict(c, wgt=np.ones_like(c["val"]))
    conf = dict(c, wgt=1 + 2 * np.abs(c["val"]), val=np.ones_like(c["val"]))
    for route in ("auto", "segmented"):
        x, plan = _dev(c["x0"].copy()), als.Plan(c["rowptr"], f)
        als.update_block(plan, _dev(c["colidx"]), _dev(c["val"]), _dev(c["Y"]), x, LAM, 2, route)
        assert np.array_equal(_update(ones, "w0=0", f, 2, route), x.cpu().numpy()), route  # w = 1, w0 = 0: explicit
        plan.close()
        const = dict(c, own=np.full(rows, W0, np.float32), gat=np.ones(N_COLS, np.float32))
        assert np.array_equal(_update(const, "rank1", f, 2, route), _update(c, "scalar", f, 2, route)), route
    x, plan, Yg = _dev(c["x0"].copy()), als.Plan(c["rowptr"], f), _dev(c["Y"])
    als.update_implicit(plan, _dev(c["colidx"]), _dev(c["val"]), Yg, als.implicit_gram(Yg), x, LAM, 2.0, solver="block", cg_iters=2)
    assert np.array_equal(_update(conf, "scalar", f, 2, "segmented", w0=1.0), x.cpu().numpy())  # w = 1 + alpha |r|: implicit
    plan.close()
    for mode in MODES:
        want = _update(c, mode, f, 2)
        for kw in ({"cuts": [0, rows // 3, 2 * rows // 3, rows]}, {"chunk": 1000}):
            assert np.array_equal(_update(c, mode, f, 2, **kw), want), (mode, kw)
    assert np.array_equal(_update(c, "w0=0", f, 2, "segmented"), _update(c, "w0=0", f, 2))


@pytest.mark.parametrize("mode", ["scalar", "rank1"])
def test_weighted_block_engine(alslib, mode):
    """Two iterations of WeightedALSEngine(solver="block") against the same recurrence in numpy on both sides; loss() against
    the reference objective of the engine's own factors, and not increasing."""
    from cumf_als_amd import als, datagen

    f = 66
    r = datagen.synth_ratings(300, 200, 6000, 100, seed=5)
    d, rng = r.numpy(), np.random.RandomState(11)
    w = rng.choice(np.array([0, 0.25, 0.5, 1.0, 2.0, 4.0], np.float32), len(d["csr_data"]))
    # the largest weight of either vector is exactly 1, so the engine's scaling of each half's pair changes nothing
    a, g = rng.uniform(0.2, 1.0, 300).astype(np.float32), rng.uniform(0.0, 1.0, 200).astype(np.float32)
    a, g = a / a.max(), g / g.max()
    kw = {"w0": W0} if mode == "scalar" else {"unobserved": (_dev(a), _dev(g))}
    for bad in ({"f": 514}, {"cg_iters": 0}, {"solver": "lu"}):
        with pytest.raises(ValueError):
            als.WeightedALSEngine(r.to("cuda"), _dev(w), **{"f": f, "lambda_": LAM, "solver": "block", **kw, **bad})
    e = als.WeightedALSEngine(r.to("cuda"), _dev(w), f, LAM, solver="block", cg_iters=1, x_batch=3, chunk=1000, **kw)
    e.init_factors(seed=1)
    csr = (d["csr_indptr"], d["csr_indices"], d["csr_data"], w)
    csc = ref.transpose(*csr, 200)
    sides = (csr, {"own": a, "gat": g}), (csc, {"own": g, "gat": a})
    out = {}
    for dtype in (np.float64, np.float32):
        X, T = e.XT.cpu().numpy().astype(dtype), e.thetaT.cpu().numpy().astype(dtype)
        for _ in range(2):
            X = block_ref(*_systems(sides[0][1], mode, T, "weighted", dtype, csr), X, 1, np.diff(csr[0]))
            T = block_ref(*_systems(sides[1][1], mode, X, "weighted", dtype, csc), T, 1, np.diff(csc[0]))
        out[dtype] = X, T
    losses = []
    for _ in range(2):
        e.iterate(1)
        X, T = e.XT.cpu().numpy(), e.thetaT.cpu().numpy()
        want = ref.sparse_loss(*csr, X, T, LAM, W0) if mode == "scalar" else ref1.sparse_loss(*csr, X, T, LAM, a, g)
        losses.append(e.loss())
        assert abs(losses[-1] - want) <= 1e-6 * abs(want), (losses, want)
    assert losses[1] <= losses[0] + 1e-6 * abs(losses[0]), losses
    for name, x, x64, x32 in zip(("X", "Theta"), (X, T), out[np.float64], out[np.float32]):
        _check(f"engine {mode} {name}", x, x64, x32, np.diff((csr if name == "X" else csc)[0]) > 0)
    e.close()


REFUSALS = [{k: None} for k in ("plan", "colidx", "val", "wgt", "gather", "update")] + [
    {"f": 6}, {"reg": 2}, {"route": 2}, {"sweeps": 0}, {"w0": -1.0}, {"w0": float("nan")}, {"G": None, "w0": W0},
    {"own": "vec"}, {"gat": "vec"}, {"own": "vec", "gat": "vec", "G": None}, {"own": "vec", "gat": "vec", "w0": W0}]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_weighted_block_refusals(alslib, capfd, bad):
    from cumf_als_amd import als

    f = bad.get("f", 64)
    rowptr = np.array([0, 2, 3], np.int32)
    start = np.random.RandomState(2).standard_normal((2, f)).astype(np.float32)
    t = {"colidx": _dev(np.array([0, 1, 1], np.int32)), "val": _dev(np.array([1.0, 2.0, 3.0], np.float32)),
         "wgt": _dev(np.array([1.0, 0.5, 2.0], np.float32)), "gather": _dev(start + 1), "update": _dev(start.copy()),
         "G": _dev(np.eye(f, dtype=np.float32)), "vec": _dev(np.ones(2, np.float32))}
    plan = als.Plan(rowptr, f)
    a = {"plan": plan._h, "own": None, "gat": None, "w0": 0.0, "reg": 0, "route": 0, "sweeps": 1,
         **{k: t[k] for k in ("colidx", "val", "wgt", "gather", "update", "G")}, **bad}
    p = {k: (t["vec"] if isinstance(v, str) else v) for k, v in a.items()}
    p = {k: (v.data_ptr() if torch.is_tensor(v) else v) for k, v in p.items()}
    assert alslib.cumf_als_update_weighted_block(p["plan"], p["colidx"], p["val"], p["wgt"], p["gather"], p["G"], p["own"], p["gat"],
                                                 p["update"], LAM, p["w0"], p["reg"], p["sweeps"], p["route"], None) == 1
    assert "cumf_als_update_weighted_block" in capfd.readouterr().err
    torch.cuda.synchronize()
    assert np.array_equal(t["update"].cpu().numpy(), start)
    plan.close()
