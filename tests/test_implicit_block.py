"""The iALS++ block solver (CUMF_SOLVER_BLOCK = 3, solver "block") without a GPU: its availability table."""
import pytest

BLOCK = 3


def test_block_availability(alslib):
    from cumf_als_amd import als

    for f in (8, 32, 34, 512):
        assert alslib.cumf_implicit_available(f, BLOCK) == 1, f
    for f in (6, 33, 514):
        assert alslib.cumf_implicit_available(f, BLOCK) == 0, f
    assert als.SOLVER_BLOCK == BLOCK and als.implicit_available(64, "block") and als.implicit_available(510, BLOCK)
    with pytest.raises(ValueError):
        als._solver_id("block")  # the explicit paths do not know it
