"""Non-negative least squares without a GPU: the C ABI of include/cumf_nnls_capi.h is exported and listed, its scope
checks, and self-checks of the fp64 reference (tests/nnls_ref.py) that tests/test_nnls_gpu.py measures against: the
reference itself, its step-by-step trace, and the cycling fixture of tests/golden with the conditions under which
tests/test_nnls_seams_gpu.py may expect the GPU solver to take exactly the trace's steps."""
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import nnls_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIP_INVALID_VALUE = 1


def test_nnls_header_symbols_are_exported(alslib):
    from cumf_als_amd import lib

    text = open(os.path.join(ROOT, "include", "cumf_nnls_capi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(cumf_[A-Za-z0-9_]+)\s*\(", text)))
    assert declared and set(declared) == set(lib.NNLS_SYMBOLS), (declared, lib.NNLS_SYMBOLS)
    for s in declared:
        assert hasattr(alslib, s), s


def test_nnls_available_table(alslib):
    for f in (0, 1, 128, 129):
        assert alslib.cumf_nnls_available(f) == int(1 <= f <= 128), f


def test_nnls_scope_refusals(alslib):
    """Refused before anything touches a device: f outside the scope, negative max_iters, no plan."""
    for f in (0, 129, -3):
        assert alslib.cumf_nnls_solve_batched(None, None, None, 4, f, 0, None, None) == HIP_INVALID_VALUE, f
    assert alslib.cumf_nnls_solve_batched(None, None, None, 4, 16, -1, None, None) == HIP_INVALID_VALUE
    assert alslib.cumf_nnls_solve_batched(None, None, None, 0, 16, 0, None, None) == 0  # an empty batch is no work
    for f in (6, 7, 9, 130, 200, 64):  # f = 64 is in scope, but there is no plan
        assert alslib.cumf_als_update_nonneg(None, None, None, None, None, f, 0.1, 0, None, None) == HIP_INVALID_VALUE
        assert alslib.cumf_als_update_implicit_nonneg(None, None, None, None, None, None, f, 0.1, 1.0, 0, 0, None,
                                                      None) == HIP_INVALID_VALUE


def test_engine_refuses_f_outside_the_nnls_scope():
    from cumf_als_amd import als

    for f in (6, 7, 130):
        with pytest.raises(ValueError):
            als.ALSEngine(None, f, 0.1, nonnegative=True)
        with pytest.raises(ValueError):
            als.ImplicitALSEngine(None, f, 0.1, 1.0, nonnegative=True)


def _case(rng, f, shift=0.0):
    A = ref.random_spd(rng, 1, f, dtype=np.float64)[0]
    b = rng.standard_normal(f) + shift
    return A, b


@pytest.mark.parametrize("f", [1, 2, 3, 5, 8, 10])
def test_reference_matches_brute_force(f):
    rng = np.random.RandomState(f)
    for _ in range(20):
        A, b = _case(rng, f)
        x, F = ref.nnls(A, b)
        xb = ref.brute_force(A, b)
        assert np.abs(x - xb).max() <= 1e-10 * max(1.0, np.abs(xb).max()), (f, x, xb)
        assert (x >= 0).all() and not (x[~F] != 0).any()


@pytest.mark.parametrize("f", [1, 2, 3, 5, 8, 10])
def test_trace_ends_where_the_reference_ends(f):
    """nnls_trace (signs against zero) on the brute-force cases: nnls's (x, F), consistent per-step records, and a warm
    start from the final passive set converges in one step."""
    rng = np.random.RandomState(f)
    for _ in range(20):
        A, b = _case(rng, f)
        x, F = ref.nnls(A, b)
        t = ref.nnls_trace(A, b)
        assert t.converged and np.array_equal(t.F, F) and np.array_equal(t.x, x), (f, t.F, F)
        assert not t.steps[0].F.any() and not t.steps[-1].V.any() and t.margin > 0
        assert t.factorisations == sum(bool(s.F.any()) for s in t.steps)
        for s, nxt in zip(t.steps, t.steps[1:]):
            flip = s.F ^ nxt.F
            assert s.V.any()
            if s.murty:
                assert flip.sum() == 1 and flip[s.index] and s.index == np.nonzero(s.V)[0].max()
            else:
                assert np.array_equal(flip, s.V) and s.index is None
        w = ref.nnls_trace(A, b, F0=F)
        assert w.converged and len(w.steps) == 1 and w.factorisations == int(F.any()) and np.array_equal(w.x, x)
        assert not ref.nnls_trace(A, b, max_steps=1).converged or len(t.steps) == 1


def _generator():
    spec = importlib.util.spec_from_file_location("make_nnls_cycling", os.path.join(GOLDEN, "make_nnls_cycling.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _cycling_traces():
    fx = ref.load_cycling()
    return fx, [ref.nnls_trace(A, b) for A, b in zip(fx["A"], fx["b"])]


def test_cycling_fixture_meets_its_conditions():
    """Every case of tests/golden/nnls_cycling.npz is the draw its generator says, and its fp64 trace from a cold start
    converges, takes a Murty step, has margin >= 2e-3 and cond_2(A) <= 2e3; the recorded counts are the trace's."""
    gen = _generator()
    fx, traces = _cycling_traces()
    assert fx["A"].dtype == np.float32 and fx["b"].dtype == np.float32 and fx["A"].shape[1:] == (8, 8)
    murty = np.array([sum(s.murty for s in t.steps) for t in traces])
    assert len(traces) >= 12 and (murty >= 3).sum() >= 3, murty
    for k, t in enumerate(traces):
        A, b = gen.draw(int(fx["draw"][k]))
        assert np.array_equal(A, fx["A"][k]) and np.array_equal(b, fx["b"][k]), k
        assert np.array_equal(A, A.T)
        assert t.converged and murty[k] >= 1 and t.margin >= gen.MARGIN, (k, t.margin)
        assert np.linalg.cond(A.astype(np.float64), 2) <= gen.COND, k
        assert gen.accept(A, b) is not None
        assert (len(t.steps), murty[k], t.factorisations) == (fx["steps"][k], fx["murty_steps"][k], fx["factorisations"][k])
        assert t.margin == fx["margin"][k]
    assert os.path.getsize(os.path.join(GOLDEN, "nnls_cycling.npz")) < 16384


def test_cycling_writer_is_deterministic(tmp_path):
    """The fixture file is its arrays alone (no clock, no compression): written again, the same bytes."""
    gen = _generator()
    fx = ref.load_cycling()
    p = tmp_path / "again.npz"
    gen.write_npz(str(p), {k: fx[k] for k in fx.files})
    assert p.read_bytes() == open(os.path.join(GOLDEN, "nnls_cycling.npz"), "rb").read()


def test_cycling_cases_need_the_backup_rule():
    """What makes the exact factorisation count of the GPU tests a test of Murty's rule: with the rule disabled (always
    the full exchange) a case either never converges or takes another number of factorisations."""
    fx, traces = _cycling_traces()
    keep = ref.cycling_needs_murty()
    assert len(keep) == len(traces) and keep.sum() >= 10, keep
    for k, t in enumerate(traces):
        u = ref.nnls_trace(fx["A"][k], fx["b"][k], murty=False)
        assert keep[k] == (not u.converged or u.factorisations != t.factorisations)
        assert not any(s.murty for s in u.steps)
    print(f"{int(keep.sum())} of {len(keep)} cases tell the schedules apart")


def test_cycling_pairs_reach_both_forms_of_the_murty_step():
    """The GPU solver keeps the infeasible set in two words, V0 for indices below 64 and V1 from 64 on, and its Murty
    step takes the top bit of V1, or of V0 when V1 is empty.  The embeddings put every Murty flip of the fixture in V0
    (block below 64), in V1 (block from 64 on), and at o = 60 some in each."""
    _, traces = _cycling_traces()
    flips = [s.index for t in traces for s in t.steps if s.murty]
    pairs = ref.CYCLING_PAIRS
    assert all(o + 8 <= f for f, o in pairs)
    assert any(o + 8 <= 64 for _, o in pairs) and any(o >= 64 for _, o in pairs)
    across = [o for _, o in pairs if o < 64 < o + 8]
    assert across and all(min(flips) + o < 64 <= max(flips) + o for o in across)


@pytest.mark.parametrize("f,o", ref.CYCLING_PAIRS)
def test_cycling_embedding_keeps_the_schedule(f, o):
    """The embedded system takes exactly the block's steps, in fp64 and in the fp32 emulation of the GPU solver's step:
    the same passive sets, Murty indices (shifted by o) and factorisation count, nothing outside the block ever moves."""
    fx, traces = _cycling_traces()
    for k, t in enumerate(traces):
        A, b = ref.embed(fx["A"][k], fx["b"][k], f, o)
        assert A.dtype == np.float32 and np.array_equal(A, A.T)
        assert A.diagonal().max() == fx["A"][k].diagonal().max() and np.abs(b).max() == np.abs(fx["b"][k]).max()
        for what, e in (("fp64", ref.nnls_trace(A, b)), ("fp32", ref.nnls_trace_fp32(A, b))):
            assert e.converged and len(e.steps) == len(t.steps) and e.factorisations == t.factorisations, (what, k)
            for se, sb in zip(e.steps, t.steps):
                inside = np.zeros(f, bool)
                inside[o:o + 8] = True
                assert not se.F[~inside].any() and not se.V[~inside].any(), (what, k)
                assert np.array_equal(se.F[inside], sb.F) and np.array_equal(se.V[inside], sb.V), (what, k)
                assert se.murty == sb.murty and se.index == (o + sb.index if sb.murty else None), (what, k)
            assert np.array_equal(e.F[o:o + 8], t.F)
        e = ref.nnls_trace(A, b)
        assert np.array_equal(e.x[o:o + 8], t.x)  # the same 8 x 8 solves
        # outside the block |y| / s = c / s; inside, y = A x - b is summed over f terms instead of 8
        assert 2e-3 <= e.margin <= t.margin * (1 + 1e-12), (k, e.margin, t.margin)


@pytest.mark.parametrize("f", [4, 16, 50])
def test_reference_matches_scipy(f):
    so = pytest.importorskip("scipy.optimize")
    rng = np.random.RandomState(100 + f)
    for _ in range(10):
        A, b = _case(rng, f)
        # 1/2 x^T A x - b^T x = 1/2 |L^T x - L^-1 b|^2 + const with A = L L^T
        L = np.linalg.cholesky(A)
        xs, _ = so.nnls(L.T, np.linalg.solve(L, b))
        x, _ = ref.nnls(A, b)
        assert np.abs(x - xs).max() <= 1e-8 * max(1.0, np.abs(xs).max()), (f, np.abs(x - xs).max())


def test_reference_positive_and_nonpositive_cases():
    rng = np.random.RandomState(5)
    for f in (3, 17, 40):
        A = ref.random_spd(rng, 1, f, dtype=np.float64)[0]
        x0 = rng.uniform(0.5, 2.0, f)  # an all-positive unconstrained solution is returned unchanged
        x, F = ref.nnls(A, A @ x0)
        assert F.all() and np.abs(x - x0).max() <= 1e-10 * np.abs(x0).max()
        x, F = ref.nnls(A, -np.abs(rng.standard_normal(f)))  # b <= 0: x = 0
        assert not F.any() and not x.any()


def test_masked_system_solution_is_the_passive_solution():
    rng = np.random.RandomState(8)
    A, b = _case(rng, 12)
    x, F = ref.nnls(A, b)
    Am, bm = ref.masked_system(A, b, F)
    xm = np.linalg.solve(Am, bm)
    assert not xm[~F].any() and np.abs(xm - x).max() <= 1e-10 * max(1.0, np.abs(x).max())
