"""Every route of the explicit CG (solver "cg" of als.update_fused, and als.cg_solve) after ONE and after TWO steps, row by row
against the plain fp64 recurrence: cg_wave_core<NB, 1, 0> at both edges of every block count NB = 2..7, cg_wave_core<NB, 2, W>
at NB = 8..13, the slot CG cg_wave_body behind chunked rows, the workgroup CG of als_item_kernel / als_reduce_kernel (f <= 14,
chunked rows at f = 112..128, Gram mode "exact"), als_short_cg_kernel at every row length 0..32, and the two batched CGs on
materialised systems.  One step does not depend on the exit test, so nothing is excluded; two steps test beta, the update of p
and the exit comparison, under a condition that each case asserts in fp64 first (tests/cg_steps_ref.py, proved on the CPU by
tests/test_cg_steps.py).  The rule is _check_rows of tests/test_implicit_seams_gpu.py with the reference's NaN for the row
without ratings: per row, max-norm distance to fp64 <= c x the fp32 oracle's largest row error + 1e-5 of the scale.

Each case covers its rows with up to three plans -- the rows of at most 32 ratings, the longer whole rows, the chunked rows --
so that the Gram kernel named after each call is the one that served that group, and asserts that the rows outside a plan's
range keep their bits.  als.last_kernel_name() names Gram(+solve) kernels only: als_short_cg_kernel, als_wave_cg_kernel and
als_reduce_kernel are launched without a note.  The short kernel is recognised by the name NOT changing over a call whose
rows all changed; the solver behind the chunk items follows from the route (als_route.cpp) and is listed in
profiles/cg_steps/README.md."""
import numpy as np
import pytest
import torch

from tests import cg_steps_ref as ref

pytestmark = pytest.mark.gpu

LENS, ROWS, LAM = ref.LENS, ref.ROWS, ref.LAM
# The constant of the rule: 1.05, the suite's value.  It holds on every route (profiles/cg_steps/README.md has the measured
# HIP / oracle32 ratios: at most 1.95, where both errors are 1e-7 and the 1e-5-of-scale term carries the bound).
C = 1.05


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared inputs are read-only


def _targs(name):
    """("als_wave_kernel", ["7", "0", "100", "3", "false"]) of "cumf::als_wave_kernel<7, 0, 100, 3, false>"."""
    assert "<" in name, name
    return name[:name.index("<")].split("::")[-1], name[name.index("<") + 1:name.rindex(">")].split(", ")


def _expected_kernel(f, exact, chunked_plan):
    """The Gram kernel of a CG half-iteration (als_route.cpp) with the 400-row table of these tests, as (base name, {template
    argument index: value}).  One wave: als_wave_kernel<NB, MODE = 0, FC, ARITH>, ARITH 3 = pre-split planes with the last block
    packed (f = 96, 100: the planes of a 400-row table fit the cache budget), 4 = in-kernel split with the rating-only last
    block packed (f % 16 == 0), 0 = in-kernel split.  Two waves: als_wave_multi_kernel<NB, 2, MODE, ARITH>, MODE 1 for chunk
    items (they only dump their tiles), ARITH 2 = pre-split planes (f % 4 == 0 and f % 16 <= 8), else 0."""
    nb = f // 16 + 1
    if exact or f <= 14:
        return "als_item_kernel", {0: nb, 2: 0}
    if nb <= 7:
        arith = 3 if f in (96, 100) else 4 if f % 16 == 0 else 0
        return "als_wave_kernel", {0: nb, 1: 0, 2: 100 if f == 100 else 0, 3: arith}
    arith = 2 if f % 4 == 0 and f % 16 <= 8 else 0
    return "als_wave_multi_kernel", {0: nb, 1: 2, 2: 1 if chunked_plan else 0, 3: arith}


def _assert_kernel(name, want, tag):
    base, args = _targs(name)
    assert base == want[0], (tag, name, want)
    for i, v in want[1].items():
        assert args[i] == str(v), (tag, name, want)


def _groups(chunk):
    """The row ranges of the three plans of a case: rows of at most 32 ratings, longer whole rows, chunked rows (LENS is
    ascending).  chunk = 0: the plan's default, which is far above 300."""
    limit = chunk if chunk > 0 else 1 << 30
    n_short, n_whole = int((LENS <= 32).sum()), int((LENS <= limit).sum())
    out = [("short", 0, n_short), ("whole", n_short, n_whole), ("chunked", n_whole, ROWS)]
    return [g for g in out if g[2] > g[1]]


class _Side:
    """The device copies that the calls of one f share."""

    def __init__(self, oracle, f):
        self.f = f
        self.rowptr, colidx, val = ref.rows()
        self.colidx, self.val, self.table = _dev(colidx), _dev(val), _dev(ref.table(f))
        self.x0 = ref.warm_start(oracle, f)

    def plan(self, a, b, chunk):
        from cumf_als_amd import als

        return als.Plan(self.rowptr, self.f, row_begin=a, row_end=b, chunk=chunk)

    def update(self, plan, iters, sse=False):
        """x0 updated through `plan`: x (all rows), the kernel name after the call, and the train SSE when asked for."""
        from cumf_als_amd import als

        x = _dev(self.x0.copy())
        bins = None
        if sse:
            bins = als.update_fused_sse(plan, self.colidx, self.val, self.table, x, LAM, "cg", iters)
        else:
            als.update_fused(plan, self.colidx, self.val, self.table, x, LAM, "cg", iters)
        torch.cuda.synchronize()
        return x.cpu().numpy(), als.last_kernel_name(), (float(bins.sum().item()) if sse else None)

    def set_sentinel(self, row):
        """Leaves a Gram kernel name that no CG call produces (the materialising pass, MODE = 2) and returns it."""
        from cumf_als_amd import als

        plan = self.plan(row, row + 1, 0)
        als.get_hermitian(plan, self.colidx, self.val, self.table, LAM)
        torch.cuda.synchronize()
        plan.close()
        return als.last_kernel_name()


class _Report:
    """Every figure of a case is printed before the case asserts: one failing row does not hide the others."""

    def __init__(self, route):
        self.route, self.bad, self.worst = route, [], 0.0

    def rows(self, x, x64, x32, a, b, tag):
        """Rows [a, b) each on its own: the NaN pattern of the reference exactly (the row without ratings), and the max-norm
        distance to fp64 within c x the fp32 oracle's largest row error in these rows + 1e-5 of their scale."""
        x, x64, x32 = x[a:b], x64[a:b], x32[a:b]
        nan = np.isnan(x64)
        if not np.array_equal(np.isnan(x), nan) or not np.array_equal(np.isnan(x32), nan):
            self.bad.append((tag, "NaN pattern", np.flatnonzero((np.isnan(x) != nan).any(1)) + a))
            return
        assert np.array_equal(nan.any(1), LENS[a:b] == 0) and np.array_equal(nan.any(1), nan.all(1)), tag
        fin = ~nan.any(1)
        if not fin.any():
            return
        scale = np.abs(x64[fin]).max()
        e_h, e_o = np.abs(x - x64).max(1)[fin], np.abs(x32 - x64).max(1)[fin]
        ratio = e_h.max() / e_o.max()
        self.worst = max(self.worst, ratio)
        bound = C * e_o.max() + 1e-5 * scale
        print(f"cg steps [{self.route}] {tag}: hip max {e_h.max():.3e} oracle32 max {e_o.max():.3e} ratio {ratio:.3f} "
              f"scale {scale:.3g} worst row / bound {e_h.max() / bound:.3f}")
        bad = np.flatnonzero(e_h > bound)
        if len(bad):
            self.bad.append((tag, np.flatnonzero(fin)[bad] + a, e_h[bad], float(e_o.max()), float(scale)))

    def exit_bits(self, x1, x2, steps, a, b, tag):
        """The exit comparison itself: a row that fp64 ends at step 1 comes back from the two-step call with the bits of the
        one-step call, every other row with ratings has moved on."""
        ended, live = steps[a:b] == 1, LENS[a:b] > 0
        same = (x1[a:b] == x2[a:b]).all(1)
        self.note(same[ended].all(), tag, "a row that ended at step 1 was touched again", np.flatnonzero(ended & ~same) + a)
        self.note(not same[live & ~ended].any(), tag, "a row took no second step", np.flatnonzero(live & ~ended & same) + a)

    def note(self, ok, *what):
        if not ok:
            self.bad.append(what)

    def done(self):
        print(f"cg steps [{self.route}]: largest hip / oracle32 ratio {self.worst:.3f} (c = {C})")
        assert not self.bad, self.bad


def _assert_exit_clear(rs1, steps, a, b, tag):
    """The condition of a two-step case, in fp64, before the GPU result is looked at: no row's r.r after step 1 within a
    factor of 4 of the exit threshold.  Rows that ended at step 1 stay in the comparison: both sides must return the
    one-step iterate there.  Every plan holds such a row (a fast row of tests/cg_steps_ref.py) and rows that go on."""
    assert ref.exit_clear(rs1[a:b]), (tag, rs1[a:b])
    ended = steps[a:b] == 1
    assert ended.any() and (steps[a:b] == 2).any() and set(np.flatnonzero(ended) + a) <= set(ref.FAST_ROWS), (tag, steps[a:b])


def _fused_case(oracle, f, chunks, route, exact=False, short_kernel=None):
    """One f through the three plans of every chunk, one and two steps, each call twice; the fused train SSE wherever the
    route offers it.  short_kernel: whether the rows of at most 32 ratings go to als_short_cg_kernel (default: on one wave
    from f = 32 on)."""
    from cumf_als_amd import als

    assert als.get_presplit() == "auto" and als.get_gram_mode() == ("exact" if exact else "auto")
    side = _Side(oracle, f)
    rep = _Report(route)
    nb = f // 16 + 1
    if short_kernel is None:
        short_kernel = not exact and 2 <= nb <= 7 and f >= 32
    for chunk in chunks:
        for group, a, b in _groups(chunk):
            plan = side.plan(a, b, chunk)
            chunked = group == "chunked"
            assert (plan.n_multi_rows == b - a) if chunked else (plan.n_multi_rows == 0), (f, chunk, group)
            if chunked:
                assert plan.n_slots == sum(-(-n // plan.chunk) for n in LENS[a:b]) and plan.chunk == chunk
            x_one = None
            for iters in ref.steps_for(f):
                tag = f"f={f} chunk={chunk} {group} rows [{a}, {b}) iters={iters}"
                x64, x32, rs1, steps = ref.fused_refs(oracle, f, iters)
                if iters == 2:
                    _assert_exit_clear(rs1, steps, a, b, tag)
                short = short_kernel and group == "short"
                sentinel = side.set_sentinel(ROWS - 1) if short else None
                x, name, _ = side.update(plan, iters)
                x2, _, _ = side.update(plan, iters)
                rep.note(np.array_equal(x, x2, equal_nan=True), tag, "two runs differ")
                rep.note(np.array_equal(x[:a], side.x0[:a]) and np.array_equal(x[b:], side.x0[b:]), tag, "rows outside moved")
                rep.note((x[a:b] != side.x0[a:b]).any(1).all(), tag, "a row inside kept its warm start")
                if short:
                    # no Gram kernel was dispatched, and every row changed: the Gram-free kernel solved them
                    assert name == sentinel and _targs(name)[1][1] == "2", (tag, name, sentinel)
                    print(f"cg steps kernel [{route}] {tag}: als_short_cg_kernel<{'true' if f > 64 else 'false'}> "
                          f"(no Gram kernel dispatched)")
                else:
                    _assert_kernel(name, _expected_kernel(f, exact, chunked), tag)
                    print(f"cg steps kernel [{route}] {tag}: {name}")
                rep.rows(x, x64, x32, a, b, tag)
                if iters == 1:
                    x_one = x
                else:
                    rep.exit_bits(x_one, x, steps, a, b, tag)
                if als.fused_sse_available(plan, "cg"):
                    xs, _, got = side.update(plan, iters, sse=True)
                    rep.note(np.array_equal(xs, x, equal_nan=True), tag, "update_fused_sse returns other factors")
                    want = ref.train_sse(x, f, a, b)
                    print(f"cg steps sse [{route}] {tag}: got {got!r} fp64 {want!r} error / bound "
                          f"{abs(got - want) / (2e-5 * want):.3f}")
                    rep.note(abs(got - want) <= 2e-5 * want, tag, "train SSE", got, want)
            plan.close()
    rep.done()


# ---- 1. the workgroup CG at NB = 1

@pytest.mark.parametrize("f", ref.F_WORKGROUP)
def test_workgroup_cg(oracle, alslib, f):
    """als_item_kernel<1, VT, CG> on whole rows and als_reduce_kernel<1, CG> behind chunk = 32; f = 2 takes one step only."""
    _fused_case(oracle, f, (0, 32), "workgroup")


# ---- 2. one wave

@pytest.mark.parametrize("f", ref.F_ONE_WAVE)
def test_one_wave_cg(oracle, alslib, f):
    """cg_wave_core<NB, 1, 0> on the accumulators (whole rows) and cg_wave_body<NB, 1, 0> on the slots (chunk = 32 and 64) at
    both edges of NB = 2..7 and at the FC = 100 instance.  Below f = 32 the rows of at most 32 ratings are whole rows of the
    wave kernel, from f = 32 on they go to the short kernel."""
    _fused_case(oracle, f, (0, 32, 64), "one wave")


# ---- 3. the short rows

@pytest.mark.parametrize("f", ref.F_SHORT)
def test_short_rows(oracle, alslib, f):
    """als_short_cg_kernel<TWO> (TWO: f > 64) with N = 8 / 16 / 32 ratings in flight: every length 1..32 is a short-kernel
    row, the row without ratings is NaN, and a row of 33 ratings is not a short row -- a plan of the rows of 0..33 ratings
    dispatches the wave kernel for it and returns the bits that the row has in a plan without short rows."""
    from cumf_als_amd import als

    _fused_case(oracle, f, (0,), "short rows", short_kernel=True)
    side = _Side(oracle, f)
    (_, a, n_short), (_, _, n_whole) = _groups(64)[:2]
    assert a == 0 and list(LENS[n_short:n_short + 1]) == [33] and n_whole > n_short + 1
    mixed, alone, shorts = side.plan(0, n_short + 1, 0), side.plan(n_short, n_short + 1, 0), side.plan(0, n_short, 0)
    for iters in (1, 2):
        sentinel = side.set_sentinel(ROWS - 1)
        x, name, _ = side.update(mixed, iters)
        assert name != sentinel, (f, name)
        _assert_kernel(name, _expected_kernel(f, False, False), f"short rows + 33, f={f}")
        xs, _, _ = side.update(shorts, iters)
        xa, _, _ = side.update(alone, iters)
        assert np.array_equal(x[:n_short], xs[:n_short], equal_nan=True) and np.array_equal(x[n_short], xa[n_short]), f
        assert np.array_equal(x[n_short + 1:], side.x0[n_short + 1:]), f
    assert als.fused_sse_available(mixed, "cg")
    for plan in (mixed, alone, shorts):
        plan.close()


# ---- 4. two waves, whole rows

@pytest.mark.parametrize("f", ref.F_TWO_WAVE)
def test_two_wave_cg(oracle, alslib, f):
    """cg_wave_core<NB, 2, W> at both edges of NB = 8..13, every row whole (the longest has 300 ratings): the lower edges on the
    pre-split planes, the upper ones on the in-kernel split (asserted from the kernel name)."""
    _fused_case(oracle, f, (0,), "two waves")


# ---- 5. chunked rows behind the two-wave Gram

@pytest.mark.parametrize("f", ref.F_TWO_WAVE_CHUNKED)
def test_two_wave_chunked_cg(oracle, alslib, f):
    """Chunk items of als_wave_multi_kernel, then als_reduce_kernel<NB, CG> (f = 112, 126, 128) or the slot CG als_wave_cg_kernel
    (f = 130 and above: one wave at NB = 9, four waves cg_wave_body<NB, 4, W> from NB = 10 on)."""
    _fused_case(oracle, f, (32, 64), "two waves, chunked" if f <= 128 else "slot cg above 128")


# ---- 6. Gram mode "exact"

@pytest.mark.parametrize("gram_mode", ["exact"], indirect=True)
@pytest.mark.parametrize("f", ref.F_EXACT)
def test_exact_mode_cg(oracle, alslib, gram_mode, f):
    """The workgroup CG on fmaf-chain tiles: the Gram has the bits of the fp32 oracle's."""
    _fused_case(oracle, f, (0, 32), "exact", exact=True)


# ---- 7. materialised systems

def _solve_case(oracle, f, half):
    from cumf_als_amd import als

    route = ("fused batched" if f <= 128 else "cg_global") + (" fp16 A" if half else "")
    rep = _Report("cg_solve " + route)
    A, b, x0 = ref.solve_inputs(oracle, f, half)
    Ag = _dev(A).half() if half else _dev(A)
    if half:
        assert np.array_equal(Ag.float().cpu().numpy(), A)  # the fp16 values are the ones the oracle ran on
    A_before, bg = Ag.clone(), _dev(b)
    for iters in ref.steps_for(f):
        tag = f"f={f} iters={iters}"
        x64, x32, rs1, steps = ref.solve_refs(oracle, f, iters, half)
        if iters == 2:
            _assert_exit_clear(rs1, steps, 0, ROWS, tag)
        got = []
        for _ in range(2):
            x = _dev(x0.copy())
            als.cg_solve(Ag, x, bg, iters)
            torch.cuda.synchronize()
            got.append(x.cpu().numpy())
        rep.note(np.array_equal(got[0], got[1], equal_nan=True), tag, "two runs differ")
        rep.note(torch.equal(Ag, A_before) and np.array_equal(bg.cpu().numpy(), b), tag, "A or b changed")
        rep.rows(got[0], x64, x32, 0, ROWS, tag)
        if iters == 1:
            x_one = got[0]
        else:
            rep.exit_bits(x_one, got[0], steps, 0, ROWS, tag)
    rep.done()


@pytest.mark.parametrize("f", ref.F_SOLVE)
def test_cg_solve(oracle, alslib, f):
    """als.cg_solve on the (A, b, x0) of the 44 rows: the LDS-resident batched CG up to f = 128, cg_global_kernel above."""
    _solve_case(oracle, f, False)


@pytest.mark.parametrize("f", ref.F_SOLVE_HALF)
def test_cg_solve_fp16_storage(oracle, alslib, f):
    """The same entry with A stored as fp16, against the oracle run on A.astype(float16).astype(float32)."""
    _solve_case(oracle, f, True)
