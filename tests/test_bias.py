"""Biased explicit ALS without a GPU: the identity the half-iteration rests on (tests/bias_ref.py, fp64), the availability
rule of the C ABI, and the separation of the reference's top-10 lists that tests/test_bias_gpu.py relies on."""
import numpy as np
import pytest

from tests import bias_ref as ref

LAM = 0.05


def test_planted_set_has_the_documented_shape():
    R, train, test = ref.planted_bias_ratings()
    assert R.shape == (300, 200) and int(train.sum()) == 7184 and int(test.sum()) == 1757
    assert not (train | test)[5].any() and not (train | test)[:, 9].any()
    assert (np.delete((train).sum(1), 5) > 0).all() and (np.delete(train.sum(0), 9) > 0).all()  # no other empty row / column


@pytest.mark.parametrize("lam_b", [LAM, LAM / 10, 10 * LAM])
def test_augmented_form_equals_the_bordered_solve(lam_b):
    """Ten alternating iterations in fp64: the F = f + 2 form on [theta | s | 0] and residual ratings against the direct
    (f + 1)-unknown solve with its own lambda_bias, to 1e-12 after every iteration."""
    data = ref.planted_bias_ratings()
    ta, td = [], []
    ref.run(10, 8, LAM, lam_b, data, ref.aug_half, ta)
    ref.run(10, 8, LAM, lam_b, data, ref.direct_half, td)
    worst = max(float(np.abs(a - d).max()) for sa, sd in zip(ta, td) for a, d in zip(sa, sd))
    print(f"lambda_bias = {lam_b}: max |augmented - direct| over 10 iterations = {worst:.3g}")
    assert worst <= 1e-12


def test_bias_model_beats_plain_width_for_width_in_fp64():
    """What the GPU end-to-end bound (0.9 x the plain engine's test RMSE) rests on: the fp64 biased model at f = 8."""
    out = ref.run(10, 8, LAM)
    print(out["train_rmse"], out["test_rmse"])
    assert abs(out["test_rmse"] - 0.2055) < 5e-4


def test_reference_top10_lists_are_separated():
    """Share of rows whose 10th and 11th best unseen reference scores differ by more than 1e-4 (measured: 0.9933): the rows on
    which the GPU test compares recommend(10) with the reference's top 10."""
    R, train, _ = ref.planted_bias_ratings()
    out = ref.run(10, 8, LAM)
    P = ref.predict(out["mu"], out["X"], out["b"], out["T"], out["c"])
    P[train] = -np.inf
    top = -np.sort(-P, axis=1)[:, :11]
    share = float(np.mean(top[:, 9] - top[:, 10] > 1e-4))
    print(f"separated rows: {share:.4f}")
    assert share >= 0.95


@pytest.mark.parametrize("f,solver,want", [(8, 1, 1), (204, 1, 1), (204, 0, 1), (7, 0, 0), (7, 1, 0), (0, 0, 0), (0, 1, 0),
                                           (206, 0, 0), (206, 1, 0)])
def test_bias_available(alslib, f, solver, want):
    assert alslib.cumf_bias_available(f, solver) == want


def test_bias_abi_is_declared_once(alslib):
    from cumf_als_amd import lib

    assert lib.ABI_BY_HEADER["cumf_bias_capi.h"] is lib.BIAS_ABI
    assert {"cumf_bias_available", "cumf_bias_update", "cumf_bias_predict", "cumf_bias_sse", "cumf_bias_mean"} <= set(lib.BIAS_ABI)
    assert all(hasattr(alslib, s) for s in lib.BIAS_SYMBOLS)
