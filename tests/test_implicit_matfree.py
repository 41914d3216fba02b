"""The matrix-free implicit CG (CUMF_SOLVER_CG_MATFREE) without a GPU: its availability table, the unchanged table of the
other two solvers, the explicit entry points refusing it, and a numpy fp64 model of the operator-only CG that equals the
oracle's CG on the materialised systems of tests/implicit_ref.py."""
import numpy as np
import pytest

from tests import implicit_ref as ref

MATFREE = 2


def test_matfree_availability(alslib):
    for f in range(8, 513, 2):
        assert alslib.cumf_implicit_available(f, MATFREE) == 1, f
    for f in (0, 6, 7, 9, 129, 514, 1000):
        assert alslib.cumf_implicit_available(f, MATFREE) == 0, f


def test_cg_and_lu_availability_is_unchanged(alslib):
    for solver in (0, 1):
        for f in range(0, 530):
            want = int(8 <= f <= 128 and f % 2 == 0)
            assert alslib.cumf_implicit_available(f, solver) == want, (f, solver)


def test_explicit_entry_points_refuse_matfree(alslib):
    for f in (16, 64, 100, 128, 200, 256):
        assert alslib.cumf_fused_available(f, 0) == int(f <= 200), f
        assert alslib.cumf_fused_available(f, MATFREE) == 0, f
        assert alslib.cumf_check_gather_table(1000, f, 0, 0) == 0, f
        assert alslib.cumf_check_gather_table(1000, f, MATFREE, 0) != 0, f


def test_python_solver_names(alslib):
    from cumf_als_amd import als

    assert als.implicit_available(256, "cg_matfree") and als.implicit_available(8, "cg_matfree")
    assert not als.implicit_available(256, "cg") and not als.implicit_available(256, "lu")
    with pytest.raises(ValueError):
        als._solver_id("cg_matfree")  # the explicit paths do not know it


def matfree_cg(rowptr, colidx, val, Y, x0, lam, alpha, reg, cg_iters):
    """The operator-only CG in fp64: A_u p = G p + T^T (w o (T p)) + reg_u p from the stored entries and G = Y^T Y, never
    forming A_u; b_u = T^T c with c = (1 + w)(r > 0).  The recurrence of oracle.cg (warm start x0, at most cg_iters steps,
    exit when r.r < 1e-4), checked per row; rows without entries get 0."""
    Y = np.asarray(Y, np.float64)
    G = Y.T @ Y
    x = np.array(x0, np.float64)
    for u in range(len(rowptr) - 1):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        if e == s:
            x[u] = 0
            continue
        T = Y[colidx[s:e]]
        r_ = np.asarray(val[s:e], np.float64)
        w = alpha * np.abs(r_)
        reg_u = ref.reg_of(e - s, lam, reg)
        op = lambda v: G @ v + T.T @ (w * (T @ v)) + reg_u * v  # noqa: E731
        b = T.T @ np.where(r_ > 0, 1 + w, 0)
        xu = x[u].copy()
        r = b - op(xu)
        p = r.copy()
        rsold = r @ r
        for _ in range(cg_iters):
            ap = op(p)
            a = rsold / (p @ ap)
            xu += a * p
            r -= a * ap
            rsnew = r @ r
            if rsnew < 1e-4:
                break
            p = r + (rsnew / rsold) * p
            rsold = rsnew
        x[u] = xu
    return x


@pytest.mark.parametrize("reg", ["weighted", "plain"])
@pytest.mark.parametrize("alpha", [1.0, 40.0])
def test_matfree_reference_equals_oracle_cg(oracle, reg, alpha):
    rng = np.random.RandomState(4)
    m, n, f = 9, 40, 6
    lens = [0, 1, 3, 7, 12, 20, 40, 5, 2]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    colidx = np.concatenate([np.sort(rng.choice(n, ln, replace=False)) for ln in lens]).astype(np.int32)
    val = rng.choice(np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0]), int(rowptr[-1]))
    Y = 0.3 * rng.standard_normal((n, f))
    x0 = 0.05 * rng.standard_normal((m, f))
    A, b = ref.systems(rowptr, colidx, val, Y, 0.05, alpha, reg)
    for iters in (0, 1, 3, 6):
        want = oracle.cg(A, x0, b, f, iters)
        want[np.asarray(lens) == 0] = 0
        got = matfree_cg(rowptr, colidx, val, Y, x0, 0.05, alpha, reg, iters)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-12), (iters, np.abs(got - want).max())
