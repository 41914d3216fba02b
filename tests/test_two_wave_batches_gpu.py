"""The two pieces of index arithmetic of the two-wave route (f = 112 .. 207) that only a plan of Netflix size used to reach.

  * The batch loop of the pooled tile buffer (two_wave_items, als_launch.cpp): the whole rows of an LU plan from f = 144 and of
    every materialising call from f = 112 go through the buffer in batches of PlanLists::part2_rows, each batch with item
    pointers moved on, mrow_row / mrow_rowlen re-pointed at the whole-row list and slots counted from the batch's first row.
    CUMF_ALS_TILE_BUFFER_GB, read at every call and honoured down to the tiles of one row, makes a buffer of exactly k rows:
    (k + 0.5) tiles' worth of bytes.  cumf_last_tile_batches must then report ceil(n_whole / k) batches of k rows -- a value
    that is ignored fails there instead of passing on one batch -- and x, tt and rhs must carry the bits of the one-batch call.
  * The role rotation of the accumulator LU (wave_role, als_kernels.hip): (index >> 8) + (index >> 10) turns the four wave
    roles with the item index (als_item_kernel) or the row index (als_reduce_kernel).  1 280 rows that repeat 16 patterns meet
    rotations 0, 1, 2, 3 and, through the >> 10 term, 1 again: every row must carry the bits of its pattern's first row.

Inputs: a gather table 0.2 * U[0, 1) of 400 rows, ratings 1 .. 5, lambda = 0.05, distinct columns per row.  Every output tensor is
pre-filled with a sentinel, so a row the loop skipped fails the comparison instead of keeping a plausible value.

Bounds (the project's own for the same quantities): LU against the oracle 1e-4 max|x_o| (test_fused_half_iteration); materialised
systems against the fp64 Gram 1e-6 max|G| and 2e-6 max|b|, and no worse than 1.5 x the exact mode's own distance + 5e-8
(test_split_gram_error_class); fused train SSE against the oracle's fp64 evaluation on the returned factors 2e-5
(test_fused_train_sse_large_f_and_chunked_rows), meaningful because the SSE is a visible share of sum r^2: rows of 300 ratings on
at most 206 features leave SSE / sum r^2 = 0.15 .. 0.17 (asserted >= 1e-2 on the oracle's factors, the rule of
test_solver_seams_gpu.py).  Between the batched and the one-batch call: bit equality, except the SSE bins -- fp64 atomics whose
grouping follows the block index, at most 15 addends per call here: 1e-10 relative (re-association is below 1e-14 of the addends,
and the SSE floor rules out cancellation).

Plan B differs from the letter of its description in one point.  It asks for rows of 300 ratings that stay whole next to rows of 200
ratings cut at chunk = 64, but one plan has one chunk size and cuts every row longer than it: at chunk = 64 the rows of 300 would
be chunked too, and rows of at most 64 ratings on f >= 130 fit perfectly (no SSE floor).  So the plan is cut at chunk = 320, the
rows of 300 stay whole and the three chunked rows have 330, 365 and 400 ratings (two slots each, 320 + the rest); everything
asserted is as described.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LAM = 0.05
TABLE_ROWS = 400
SENTINEL = 777.0
ENV = "CUMF_ALS_TILE_BUFFER_GB"

_cache = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _table(f):
    if ("table", f) not in _cache:
        rng = np.random.RandomState(1)
        _cache["table", f], = _frozen((0.2 * rng.random_sample((TABLE_ROWS, f))).astype(np.float32))
    return _cache["table", f]


def _csr(lens, seed):
    """(row pointer, columns, ratings, row of every entry) of rows with the given lengths: distinct sorted columns, ratings 1 .. 5."""
    rng = np.random.RandomState(seed)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(TABLE_ROWS, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.randint(1, 6, size=len(idx)).astype(np.float32)
    row = np.repeat(np.arange(len(lens)), lens).astype(np.int32)
    return _frozen(ptr, idx, val, row)


# Plan A: 12 whole rows of 300 ratings, one row of 1 rating, one row of none.
A_LENS = [300] * 12 + [1, 0]
# Plan B, a window [4, 15) of 20 rows: inside it 6 rows of 300, the row of 1, the empty row and three rows longer than the chunk;
# outside it rows with ratings that the plan must not touch.
B_CHUNK = 320
B_LENS = [300, 400, 300, 300] + [300, 330, 300, 1, 300, 365, 300, 0, 300, 400, 300] + [300, 350, 300, 300, 300]
B_BEGIN, B_END = 4, 15
# ... and a plan whose rows are all chunked
C_LENS = [330, 400, 365, 321, 390]


def _plan_data(kind):
    if ("csr", kind) not in _cache:
        lens, seed = {"A": (A_LENS, 11), "B": (B_LENS, 12), "chunked": (C_LENS, 13)}[kind]
        _cache["csr", kind] = _csr(lens, seed)
    return _cache["csr", kind]


def _window(kind):
    """(row_begin, row_end, chunk, whole rows of the plan)"""
    if kind == "A":
        return 0, len(A_LENS), 0, len(A_LENS)
    if kind == "B":
        return B_BEGIN, B_END, B_CHUNK, sum(n <= B_CHUNK for n in B_LENS[B_BEGIN:B_END])
    return 0, len(C_LENS), B_CHUNK, 0


def _oracle_lu(oracle, kind, f):
    """The oracle's fp32 LU half-iteration on ALL rows of the data, its fp64 SSE over the plan's entries and their sum r^2."""
    if ("lu", kind, f) not in _cache:
        ptr, idx, val, row = _plan_data(kind)
        b, e, _, _ = _window(kind)
        x_o = oracle.half_iteration(ptr, idx, val, _table(f), np.zeros((len(ptr) - 1, f), np.float32), f, LAM, solver="lu")
        sl = slice(int(ptr[b]), int(ptr[e]))
        sse = oracle.sse(val[sl], row[sl], idx[sl], _table(f), x_o, sl.stop - sl.start, f, dtype=np.float64)
        _cache["lu", kind, f] = (_frozen(x_o)[0], float(sse), float((val[sl].astype(np.float64) ** 2).sum()))
    return _cache["lu", kind, f]


def _oracle_gram(oracle, kind, f):
    """fp64 Gram + right-hand sides of the plan's rows."""
    if ("gram", kind, f) not in _cache:
        ptr, idx, val, _ = _plan_data(kind)
        b, e, _, _ = _window(kind)
        _cache["gram", kind, f] = _frozen(*oracle.gram_rhs(ptr, idx, val, _table(f), f, LAM, row_begin=b, row_end=e,
                                                          dtype=np.float64))
    return _cache["gram", kind, f]


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _buffer_gb(k, f):
    nb = f // 16 + 1
    return repr((k + 0.5) * nb * (nb + 1) / 2 * 1024 / 2 ** 30)


def _expect_batches(n_whole, k=None):
    """What cumf_last_tile_batches must report for n_whole rows through a buffer of k rows (None: the default sizing)."""
    if n_whole == 0:
        return (0, 0)
    rows = n_whole if k is None else min(k, n_whole)
    return (math.ceil(n_whole / rows), rows)


def _both_sizings(call, monkeypatch, f, k, n_whole):
    """call() under the default sizing (one batch) and with a buffer of exactly k rows; the probe is asserted after each."""
    from cumf_als_amd import als

    monkeypatch.delenv(ENV, raising=False)
    one = call()
    got = als.last_tile_batches()
    assert got == _expect_batches(n_whole), ("default sizing", got)
    monkeypatch.setenv(ENV, _buffer_gb(k, f))
    many = call()
    got = als.last_tile_batches()
    assert got == _expect_batches(n_whole, k), (f"buffer of {k} rows", got, _expect_batches(n_whole, k))
    monkeypatch.delenv(ENV, raising=False)
    return one, many


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared inputs are read-only


def _lu_call(kind, f):
    """update_fused_sse (LU) on a sentinel-filled update tensor -> (x on the host, its bits, SSE of the bins)."""
    from cumf_als_amd import als

    ptr, idx, val, _ = _plan_data(kind)
    b, e, chunk, _ = _window(kind)
    plan = als.Plan(ptr, f, row_begin=b, row_end=e, chunk=chunk)
    assert als.fused_sse_available(plan, "lu")
    gi, gv, gt = _dev(idx), _dev(val), _dev(_table(f))

    def call():
        x = torch.full((len(ptr) - 1, f), SENTINEL, device="cuda")
        bins = als.update_fused_sse(plan, gi, gv, gt, x, LAM, "lu")
        torch.cuda.synchronize()
        return x.cpu().numpy(), _bits(x), float(bins.sum().item())

    return plan, call


def _check_lu(oracle, kind, f, one, many, label):
    ptr, idx, val, row = _plan_data(kind)
    b, e, _, _ = _window(kind)
    x_o, sse_o, s2 = _oracle_lu(oracle, kind, f)
    (x1, bits1, sse1), (xk, bitsk, ssek) = one, many
    inside = np.zeros(len(ptr) - 1, bool)
    inside[b:e] = True
    keep = inside & (np.diff(ptr) > 0)
    empty = inside & (np.diff(ptr) == 0)
    err = np.abs(x1[keep] - x_o[keep]).max()
    sl = slice(int(ptr[b]), int(ptr[e]))
    ref = float(oracle.sse(val[sl], row[sl], idx[sl], _table(f), x1, sl.stop - sl.start, f, dtype=np.float64))
    print(f"{label}: SSE share of the oracle's factors {sse_o / s2:.4f}; max|x - x_o| = {err:.3e} (max|x_o| = "
          f"{np.abs(x_o[keep]).max():.3e}); fused SSE {sse1:.6f} vs fp64 {ref:.6f} rel {abs(sse1 - ref) / ref:.2e}; "
          f"batched SSE rel {abs(ssek - sse1) / sse1:.2e}; bits equal {np.array_equal(bitsk, bits1)}")
    assert sse_o >= 1e-2 * s2, (sse_o, s2)
    # the batched call against the one-batch call
    np.testing.assert_array_equal(bitsk, bits1)
    assert abs(ssek - sse1) <= 1e-10 * sse1, (ssek, sse1)
    # the one-batch call against the oracle
    assert (x1[~inside] == SENTINEL).all(), "a row outside the plan was written"
    assert empty.sum() == (1 if kind != "chunked" else 0)
    assert np.array_equal(np.isnan(x1[inside]), np.isnan(x_o[inside])) and np.isnan(x1[empty]).all()
    assert err <= 1e-4 * np.abs(x_o[keep]).max(), err
    assert abs(sse1 - ref) <= 2e-5 * ref, (sse1, ref)


def _triu(f):
    return np.triu_indices(f)


def _mat_call(kind, f, packed):
    from cumf_als_amd import als

    ptr, idx, val, _ = _plan_data(kind)
    b, e, chunk, _ = _window(kind)
    plan = als.Plan(ptr, f, row_begin=b, row_end=e, chunk=chunk)
    gi, gv, gt = _dev(idx), _dev(val), _dev(_table(f))
    rows = e - b

    def call():
        tt = torch.full((rows, f * (f + 1) // 2) if packed else (rows, f, f), SENTINEL, device="cuda")
        rhs = torch.full((rows, f), SENTINEL, device="cuda")
        (als.get_hermitian_packed if packed else als.get_hermitian)(plan, gi, gv, gt, LAM, tt, rhs)
        torch.cuda.synchronize()
        return tt.cpu().numpy(), rhs.cpu().numpy(), _bits(tt), _bits(rhs)

    return plan, call


def _exact_mode_errors(oracle, kind, f):
    """Distance of gram mode exact (the fmaf chain) from the fp64 systems of the plan: the yardstick of test_split_gram_error_class."""
    from cumf_als_amd import als

    if ("exact", kind, f) not in _cache:
        tt64, b64 = _oracle_gram(oracle, kind, f)
        als.set_gram_mode("exact")
        try:
            _, call = _mat_call(kind, f, False)
            tt, rhs, _, _ = call()
        finally:
            als.set_gram_mode("auto")
        _cache["exact", kind, f] = (np.abs(tt - tt64).max() / np.abs(tt64).max(), np.abs(rhs - b64).max() / np.abs(b64).max())
    return _cache["exact", kind, f]


def _check_mat(oracle, kind, f, packed, one, many, label):
    tt64, b64 = _oracle_gram(oracle, kind, f)
    if packed:
        iu = _triu(f)
        tt64 = tt64[:, iu[0], iu[1]]
    (tt1, rhs1, tbits1, rbits1), (_, _, tbitsk, rbitsk) = one, many
    e_tt, e_rhs = np.abs(tt1 - tt64).max() / np.abs(tt64).max(), np.abs(rhs1 - b64).max() / np.abs(b64).max()
    x_tt, x_rhs = _exact_mode_errors(oracle, kind, f)
    print(f"{label}: |tt - tt64| / max = {e_tt:.3e} (exact mode {x_tt:.3e}), |rhs - b64| / max = {e_rhs:.3e} (exact mode "
          f"{x_rhs:.3e}); bits equal {np.array_equal(tbitsk, tbits1)} / {np.array_equal(rbitsk, rbits1)}")
    np.testing.assert_array_equal(tbitsk, tbits1)
    np.testing.assert_array_equal(rbitsk, rbits1)
    assert not (tt1 == SENTINEL).any() and not (rhs1 == SENTINEL).any(), "a system of the plan was not written"
    assert e_tt <= 1e-6 and e_rhs <= 2e-6, (e_tt, e_rhs)
    assert e_tt <= 1.5 * x_tt + 5e-8 and e_rhs <= 1.5 * x_rhs + 5e-8, (e_tt, x_tt, e_rhs, x_rhs)


# ---- A. Batches give the bits of one batch

K_A = [1, 5, 14, 15]  # 14 batches; 5 + 5 + 4; exactly one batch; a buffer larger than the plan


@pytest.mark.parametrize("k", K_A)
@pytest.mark.parametrize("f,gram_mode", [(144, "auto"), (160, "auto"), (190, "auto"), (206, "auto"), (160, "fast"), (206, "fast")],
                         indirect=["gram_mode"])
def test_lu_batches_give_the_bits_of_one_batch(oracle, alslib, gram_mode, monkeypatch, f, k):
    """cumf_als_update_fused_sse, LU, NB = 10 .. 13 (f = 144 and 160 with the pre-split planes, 190 and 206 without; 190 has
    f % 4 != 0), 14 whole rows through a buffer of 1, 5, 14 and 15 rows."""
    _need_gpu()
    _, call = _lu_call("A", f)
    one, many = _both_sizings(call, monkeypatch, f, k, len(A_LENS))
    _check_lu(oracle, "A", f, one, many, f"A lu f={f} {gram_mode} k={k}")


@pytest.mark.parametrize("k", K_A)
@pytest.mark.parametrize("f,packed", [(112, False), (130, False), (206, False), (160, True)])
def test_materialise_batches_give_the_bits_of_one_batch(oracle, alslib, gram_mode, monkeypatch, f, packed, k):
    """cumf_get_hermitian at the first f of the two-wave route, inside it and at its last even f, cumf_get_hermitian_packed at
    f = 160: the same 14 rows through the same buffers."""
    _need_gpu()
    _, call = _mat_call("A", f, packed)
    one, many = _both_sizings(call, monkeypatch, f, k, len(A_LENS))
    _check_mat(oracle, "A", f, packed, one, many, f"A materialise f={f} packed={packed} k={k}")


# ---- B. Batches with everything else in the plan

@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("f", [160, 206])
@pytest.mark.parametrize("kind", ["B", "chunked"])
def test_lu_batches_next_to_chunked_rows(oracle, alslib, gram_mode, monkeypatch, kind, f, k):
    """The chunked phase (plan slots, mrow_* of the plan) and the tile-buffer phase (dense slots, mrow_* re-pointed per batch) in
    one call, on rows [4, 15) of 20: the LU writes at the row's own index and the rows outside the plan keep the sentinel.  On a
    plan whose rows are all chunked the probe reads no batch and no buffer."""
    _need_gpu()
    plan, call = _lu_call(kind, f)
    assert plan.n_multi_rows == (3 if kind == "B" else len(C_LENS)) and plan.n_slots == 2 * plan.n_multi_rows
    one, many = _both_sizings(call, monkeypatch, f, k, _window(kind)[3])
    _check_lu(oracle, kind, f, one, many, f"{kind} lu f={f} k={k}")


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("kind", ["B", "chunked"])
def test_materialise_batches_next_to_chunked_rows(oracle, alslib, gram_mode, monkeypatch, kind, k):
    """cumf_get_hermitian at f = 130 on the same two plans: the systems are written at row - row_begin."""
    _need_gpu()
    f = 130
    plan, call = _mat_call(kind, f, False)
    assert plan.n_multi_rows == (3 if kind == "B" else len(C_LENS))
    one, many = _both_sizings(call, monkeypatch, f, k, _window(kind)[3])
    _check_mat(oracle, kind, f, False, one, many, f"{kind} materialise f={f} k={k}")


def test_default_sized_plan_after_a_one_row_buffer(oracle, alslib, gram_mode, monkeypatch):
    """The pooled buffer is grow-only and shared by every plan of the stream: after a call at NB = 11 on a buffer of one row, a
    default-sized call at NB = 13 on the same stream is the oracle's."""
    _need_gpu()
    from cumf_als_amd import als

    _, call = _lu_call("B", 160)
    monkeypatch.setenv(ENV, _buffer_gb(1, 160))
    call()
    assert als.last_tile_batches() == (8, 1)
    monkeypatch.delenv(ENV)
    _, call = _lu_call("A", 206)
    one = call()
    assert als.last_tile_batches() == (1, len(A_LENS))
    _check_lu(oracle, "A", 206, one, one, "A lu f=206 after a one-row buffer at f=160")


# ---- C. Role rotation leaves the bits alone

PATTERNS, ROT_ROWS = 16, 1280


def _rotation_data(L):
    """ROT_ROWS rows, row u with the ratings of pattern u % 16 (all of L ratings: the plan's stable longest-first order is then
    the row order, row u is launch index u)."""
    if ("rot", L) not in _cache:
        ptr16, idx16, val16, _ = _csr([L] * PATTERNS, 20 + L)
        reps = ROT_ROWS // PATTERNS
        ptr = (np.arange(ROT_ROWS + 1) * L).astype(np.int32)
        _cache["rot", L] = _frozen(ptr16, idx16, val16, ptr, np.tile(idx16, reps), np.tile(val16, reps))
    return _cache["rot", L]


def _rotation_case(oracle, f, L, chunk, label, monkeypatch, through_buffer, k=None):
    from cumf_als_amd import als

    ptr16, idx16, val16, ptr, idx, val = _rotation_data(L)
    if ("rot_lu", L, f) not in _cache:
        _cache["rot_lu", L, f], = _frozen(oracle.half_iteration(ptr16, idx16, val16, _table(f), np.zeros((PATTERNS, f), np.float32),
                                                               f, LAM, solver="lu"))
    x_o = _cache["rot_lu", L, f]
    plan = als.Plan(ptr, f, chunk=chunk)
    assert plan.n_multi_rows == (ROT_ROWS if chunk else 0) and plan.n_items == (2 if chunk else 1) * ROT_ROWS
    gi, gv, gt = _dev(idx), _dev(val), _dev(_table(f))

    def call():
        x = torch.full((ROT_ROWS, f), SENTINEL, device="cuda")
        als.update_fused(plan, gi, gv, gt, x, LAM, "lu")
        torch.cuda.synchronize()
        return x.cpu().numpy(), _bits(x)

    n_whole = ROT_ROWS if through_buffer else 0
    monkeypatch.delenv(ENV, raising=False)
    x, bits = call()
    assert als.last_tile_batches() == _expect_batches(n_whole), als.last_tile_batches()
    differ = np.nonzero((bits != np.tile(bits[:PATTERNS], (ROT_ROWS // PATTERNS, 1))).any(1))[0]
    err = np.abs(x[:PATTERNS] - x_o).max()
    print(f"{label}: rows whose bits differ from their pattern's first row: {len(differ)} {differ[:8].tolist()}; "
          f"max|x[:16] - x_o| = {err:.3e} (max|x_o| = {np.abs(x_o).max():.3e})")
    assert len(differ) == 0, (len(differ), differ[:8].tolist(), sorted(set((differ >> 8).tolist())))
    assert err <= 1e-4 * np.abs(x_o).max(), err
    if k is not None:
        monkeypatch.setenv(ENV, _buffer_gb(k, f))
        _, bits_k = call()
        got = als.last_tile_batches()
        monkeypatch.delenv(ENV)
        assert got == _expect_batches(n_whole, k), got
        np.testing.assert_array_equal(bits_k, bits)


@pytest.mark.parametrize("f,gram_mode", [(144, "auto"), (160, "auto"), (180, "auto"), (206, "auto"), (206, "fast"), (100, "exact"),
                                         (206, "exact")], indirect=["gram_mode"])
def test_role_rotation_whole_rows(oracle, alslib, gram_mode, monkeypatch, f):
    """Whole rows of 24 ratings.  Default and fast mode: als_reduce_kernel on the dense slots of the tile buffer (the blocked LU of
    NB = 10 .. 13, four workgroups per CU from NB = 11), rotated by the row's index in its batch; gram mode exact:
    als_item_kernel, rotated by the item index (NB = 7: the unblocked LU; NB = 13)."""
    _need_gpu()
    _rotation_case(oracle, f, 24, 0, f"rotation whole rows f={f} {gram_mode}", monkeypatch, through_buffer=gram_mode != "exact")


@pytest.mark.parametrize("f", [100, 112, 130, 144, 180, 206])
def test_role_rotation_chunked_rows(oracle, alslib, gram_mode, monkeypatch, f):
    """Rows of 40 ratings cut at chunk = 32 (two slots each): als_reduce_kernel on the plan's slots at NB = 7 .. 13, rotated by
    the row's index in the list of chunked rows."""
    _need_gpu()
    _rotation_case(oracle, f, 40, 32, f"rotation chunked rows f={f}", monkeypatch, through_buffer=False)


def test_role_rotation_across_batches(oracle, alslib, gram_mode, monkeypatch):
    """f = 206, batches of 300, 300, 300, 300 and 80 rows: a row's rotation is that of its index in the batch, no longer the one
    of the one-batch run, and the first row of a batch crosses 256.  The bits are those of the default-sized run."""
    _need_gpu()
    _rotation_case(oracle, 206, 24, 0, "rotation f=206 in batches of 300", monkeypatch, through_buffer=True, k=300)
