"""The matrix-free explicit half-iteration (include/cumf_free_capi.h) without a GPU: its availability table, the refusals
that touch no device, the Python names, and the numpy fp64 model of tests/free_ref.py against the oracle's CG on the
materialised systems."""
import ctypes as C

import numpy as np
import pytest

from tests import free_ref as ref


def test_matfree_availability(alslib):
    from cumf_als_amd import als

    for f in range(8, 513, 2):
        assert alslib.cumf_matfree_available(f) == 1, f
    for f in (0, 6, 7, 9, 129, 514):
        assert alslib.cumf_matfree_available(f) == 0, f
    assert als.matfree_available(8) and als.matfree_available(512) and not als.matfree_available(129)
    # the explicit entry points answer for solver 2 as before
    for f in (64, 256):
        assert alslib.cumf_fused_available(f, 2) == 0
        assert alslib.cumf_check_gather_table(1000, f, 2, 0) != 0


def test_update_matfree_refuses_null_pointers(alslib, capfd):
    """A NULL plan or pointer is refused with hipErrorInvalidValue (1) and a printed reason before any device call."""
    buf = np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)  # never dereferenced: the plan is NULL
    assert alslib.cumf_als_update_matfree(None, buf, buf, buf, buf, 0.05, 6, None) == 1
    assert "cumf_als_update_matfree" in capfd.readouterr().err
    assert alslib.cumf_als_update_matfree(None, None, None, None, None, 0.05, 6, None) == 1


def test_python_names(alslib):
    from cumf_als_amd import als

    with pytest.raises(ValueError):
        als._solver_id("cg_matfree")  # the fused and materialising entry points do not know it
    with pytest.raises(ValueError):
        als.do_als(*[None] * 10, 4, 4, 7, 0, 0, 0.05, 1, 1, 1, solver="cg_matfree")  # odd f, refused before any work
    with pytest.raises(ValueError):
        als.do_als(*[None] * 10, 4, 4, 514, 0, 0, 0.05, 1, 1, 1, solver="cg_matfree")


def _rows(rng, lens, n, f):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lens]).astype(np.int32)
    val = rng.choice(np.arange(0.5, 5.01, 0.5), int(rowptr[-1]))
    return rowptr, colidx, val


def test_matfree_reference_equals_oracle_cg(oracle):
    rng = np.random.RandomState(4)
    n, f = 40, 6
    lens = [0, 1, 3, 7, 12, 20, 40, 5, 2, 9, 30]
    rowptr, colidx, val = _rows(rng, lens, n, f)
    Y = 0.3 * rng.standard_normal((n, f))
    A, b = ref.systems(rowptr, colidx, val, Y, 0.05)
    x0 = 0.05 * rng.standard_normal((len(lens), f))
    # rows 9 and 10 start one eigenvector (two eigenvectors) of A_u away from the solution: they end at steps 1 and 2
    for u, pick in ((9, [2]), (10, [0, 5])):
        lam, U = np.linalg.eigh(A[u])
        x0[u] = np.linalg.solve(A[u], b[u]) + 3.0 * sum(U[:, i] / lam[i] for i in pick)
    empty = np.asarray(lens) == 0
    for iters in (0, 1, 3, 6):
        want = oracle.cg(A[~empty], x0[~empty], b[~empty], f, iters)  # (the oracle's 0 / 0 on an empty row: NaN)
        got, steps = ref.matfree_cg(rowptr, colidx, val, Y, x0, 0.05, iters)
        assert (got[empty] == 0).all()
        assert np.abs(got[~empty] - want).max() <= 1e-12 * np.abs(want).max(), (iters, np.abs(got[~empty] - want).max())
        if iters == 6:
            assert steps[9] == 1 and steps[10] == 2 and steps[6] > 2, steps


def test_uniform_model_equals_the_row_model():
    """free_ref.matfree_cg_uniform (all rows of one length at once) is free_ref.matfree_cg, early exits included."""
    rng = np.random.RandomState(8)
    rows, n, n_cols, f = 50, 2, 30, 8
    cols = np.stack([np.sort(rng.choice(n_cols, n, replace=False)) for _ in range(rows)]).astype(np.int32)
    vals = rng.choice(np.arange(0.5, 5.01, 0.5), (rows, n))
    Y = 0.3 * rng.standard_normal((n_cols, f))
    x0 = 0.05 * rng.standard_normal((rows, f))
    rowptr = n * np.arange(rows + 1)
    for iters in (0, 1, 2, 3, 6):
        want, steps = ref.matfree_cg(rowptr, cols.reshape(-1), vals.reshape(-1), Y, x0, 0.05, iters)
        got = ref.matfree_cg_uniform(cols, vals, Y, x0, 0.05, iters)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), iters
    assert steps.max() <= 3 < 6  # rank n + 1 systems: every row ended early
