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
