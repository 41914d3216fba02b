"""The dual-form LU of short whole rows (als_dual.hip): what a plan counts for it and when the route takes it.  Host only
(cumf_dual_rows_probe: no GPU, no plan)."""
import numpy as np
import pytest


def _rowptr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


@pytest.fixture
def als(alslib):
    from cumf_als_amd import als as mod

    yield mod
    mod.set_presplit("auto")
    mod.set_gram_mode("auto")


def test_plan_counts_for_hand_made_row_pointers(als):
    lens = [0, 1, 32, 33, 79, 80, 95, 96, 200, 0, 64]
    got = als.dual_rows_probe(_rowptr(lens), 100, 2048, "lu", gather_rows=300)
    assert got == {"rows_1_79": 5, "rows_1_95": 7, "rows_empty": 2, "routed": 5}
    # a row's own length decides: the batches of a plan add up to the whole plan
    parts = [als.dual_rows_probe(_rowptr(lens), 100, 2048, "lu", gather_rows=300, row_begin=b, row_end=e)
             for b, e in ((0, 4), (4, 8), (8, 11))]
    for key in got:
        assert sum(p[key] for p in parts) == got[key], key
    # int64 row pointers count the same
    assert als.dual_rows_probe(_rowptr(lens).astype(np.int64), 100, 2048, "lu", gather_rows=300) == got
    # a row longer than the chunk is no whole row: with chunk 64 the rows of 79 ratings are chunked
    small = als.dual_rows_probe(_rowptr([10, 79, 64, 65]), 100, 64, "lu", gather_rows=300)
    assert small["rows_1_79"] == 2 and small["rows_1_95"] == 2


def test_route_follows_the_rows_own_length(als):
    short = [40] * 100
    # no chunked rows: one launch of whole rows
    assert als.dual_rows_probe(_rowptr(short), 100, 2048, "lu", gather_rows=300)["routed"] == 100
    # a few chunked rows (< 25 % of the ratings): the chunk items go first, the whole rows keep a launch of their own
    assert als.dual_rows_probe(_rowptr(short + [1200]), 100, 1024, "lu", gather_rows=300)["routed"] == 100
    # chunks are most of the work: one combined launch of chunk items and whole rows -- the same rows are taken all the same
    assert als.dual_rows_probe(_rowptr(short + [20000]), 100, 1024, "lu", gather_rows=300)["routed"] == 100


def test_route_declines(als, monkeypatch):
    rp = _rowptr([40] * 10 + [120] * 3)

    def routed(f=100, solver="lu", materialize=False, gather_rows=300):
        return als.dual_rows_probe(rp, f, 2048, solver, materialize, gather_rows)["routed"]

    assert routed() == 10
    assert routed(f=96) == 10
    assert routed(solver="cg") == 0
    assert routed(materialize=True) == 0
    assert routed(gather_rows=0) == 0          # size of the table unknown: no pre-split table
    assert routed(gather_rows=10 ** 6) == 0    # 608 MB of planes: the table stays fp32
    assert routed(f=64) == 0 and routed(f=80) == 0 and routed(f=112) == 0
    assert routed(f=108) == 0                  # no pre-split form for a strip of twelve features
    for mode in ("off", "verify"):             # the forms the bit-identity tests compare keep their route
        als.set_presplit(mode)
        assert routed() == 0, mode
    als.set_presplit("on")
    assert routed() == 10 and routed(gather_rows=10 ** 6) == 10
    als.set_presplit("auto")
    for mode in ("exact", "fast"):
        als.set_gram_mode(mode)
        assert routed() == 0, mode
    als.set_gram_mode("auto")
    monkeypatch.setenv("CUMF_ALS_DUAL", "0")
    assert routed() == 0
    monkeypatch.setenv("CUMF_ALS_DUAL", "1")
    assert routed() == 10
    monkeypatch.delenv("CUMF_ALS_DUAL")
    assert routed() == 10
