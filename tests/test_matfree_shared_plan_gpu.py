"""One plan serving all three routes that build lists on it at first use: the explicit matrix-free CG (the row segments), the
implicit "cg" route (the long-row / empty-row lists) and the implicit matrix-free CG (both).  The segments are owned by the
plan itself, not by the implicit lists, so the order of the first uses must not matter."""
import numpy as np
import pytest
import torch

from tests import implicit_ref as ref
from tests.test_implicit_gpu import _dev, _table
from tests.test_implicit_matfree_seams_gpu import LAM, N_COLS, _seam_rows

pytestmark = pytest.mark.gpu

F, ITERS, ALPHA, REG = 66, 3, 40.0, "weighted"


def _cg_bound(x, x64, x32, lens):
    """The bound of tests/test_implicit_gpu.py::test_update_implicit_cg: rows without entries exactly 0; median / q90 / max of
    the per-row max-norm distance to the fp64 oracle.cg within 1.05 x those of the fp32 oracle.cg + 1e-5 of the scale."""
    stats = lambda v: (float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max()))
    empty = lens == 0
    assert (x[empty] == 0).all()
    e_h = np.abs(x - x64).max(1)[~empty]
    e_o = np.abs(x32 - x64).max(1)[~empty]
    scale = np.abs(x64).max()
    print(f"shared plan, implicit cg: hip {stats(e_h)} oracle32 {stats(e_o)}")
    for sh, so in zip(stats(e_h), stats(e_o)):
        assert sh <= 1.05 * so + 1e-5 * scale, (stats(e_h), stats(e_o))


def test_three_routes_share_one_plan_in_either_order(oracle, alslib):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _seam_rows()  # 45 rows of 0 ... 4097 entries: empty rows, one to three segments per row
    Y = _table(N_COLS, F, 3)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), F))).astype(np.float32)
    cg, vg, Yg = _dev(colidx), _dev(val), _dev(Y)
    G = als.implicit_gram(Yg)

    def run(plan, route):
        x = _dev(x0.copy())
        if route == "a":
            als.update_matfree(plan, cg, vg, Yg, x, LAM, ITERS)
        else:
            als.update_implicit(plan, cg, vg, Yg, G, x, LAM, ALPHA, REG, "cg" if route == "b" else "cg_matfree", ITERS)
        torch.cuda.synchronize()
        return x.cpu().numpy()

    alone = {}
    for route in "ac":  # each matrix-free route on a fresh plan of its own
        plan = als.Plan(rowptr, F)
        alone[route] = run(plan, route)
        plan.close()
    assert not np.array_equal(alone["a"], alone["c"])  # two different problems: a result cannot pass for the other's

    A64, b64 = ref.systems(rowptr, colidx, val, Y, LAM, ALPHA, REG)
    x64 = oracle.cg(A64, x0.astype(np.float64), b64, F, ITERS)
    x32 = oracle.cg(A64.astype(np.float32), x0, b64.astype(np.float32), F, ITERS)
    for order in ("abc", "cba"):
        plan = als.Plan(rowptr, F)
        for route in order:
            x = run(plan, route)
            if route == "b":
                _cg_bound(x, x64, x32, lens)
            else:
                assert np.array_equal(x.view(np.int32), alone[route].view(np.int32)), (order, route)
        plan.close()
