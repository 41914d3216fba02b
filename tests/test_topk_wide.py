"""Top-k above k = 128 without a GPU: the scope check of cumf_topk_wide (include/cumf_topk_capi.h) and its Python twin."""
import pytest


@pytest.mark.parametrize("f", [0, 1, 512, 513])
@pytest.mark.parametrize("k", [0, 1, 128, 129, 2048, 2049])
def test_topk_wide_available_table(alslib, f, k):
    from cumf_als_amd import als

    want = int(1 <= f <= 512 and 1 <= k <= 2048)
    assert alslib.cumf_topk_wide_available(f, k) == want
    assert als.topk_wide_available(f, k) is bool(want)
