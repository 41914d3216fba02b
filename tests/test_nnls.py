"""Non-negative least squares without a GPU: the C ABI of include/cumf_nnls_capi.h is exported and listed, its scope
checks, and self-checks of the fp64 reference (tests/nnls_ref.py) that tests/test_nnls_gpu.py measures against."""
import os
import re

import numpy as np
import pytest

from tests import nnls_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
