"""Routing answers that need no GPU: cumf_fused_available against the table the library gave before routing was
decided in one place (tests/golden/fused_available.json, written by tests/golden/make_fused_available.py)."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_available.json")


def test_fused_available_matches_golden_table(alslib, monkeypatch):
    from tests.golden.make_fused_available import table

    for knob in ("CUMF_ALS_GRAM", "CUMF_ALS_NO_BATCHED"):
        monkeypatch.delenv(knob, raising=False)
    assert table(alslib) == json.load(open(GOLDEN))


def test_tile_batch_probe_before_any_launch(alslib):
    """cumf_last_tile_batches is plain host state: before any half-iteration of the process it returns 0 and reports no batch
    and no buffer rows (no HIP call, no GPU needed); a null pointer is refused."""
    import ctypes as C

    info = (C.c_long * 2)(-1, -1)
    assert alslib.cumf_last_tile_batches(info) == 0
    assert (info[0], info[1]) == (0, 0)
    assert alslib.cumf_last_tile_batches(None) != 0
    from cumf_als_amd import als

    assert als.last_tile_batches() == (0, 0)
