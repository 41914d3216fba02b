"""The NNLS kernel (nnls_bpp_kernel<NB>, als_nnls.hip) at every block count, mask seam and backup step, on the MI355X.

NB = f / 16 + 1 = 1..9.  The passive set lives in two 64-bit words that split at index 64.  tests/test_nnls_gpu.py runs
f = 1, 8, 10, 16, 32, 50, 64, 100, 128; this file adds
  a  both edges of every NB (f = 16 NB - 16 and 16 NB - 1, where the right-hand side is the last column of the last
     register block) and 63 / 65, at three scales of (A, b);
  b  the pivoting schedule against the fp64 trace of tests/nnls_ref.py on the systems of tests/golden/nnls_cycling.npz,
     which reach Murty's backup rule, embedded below, across and above the split: the factorisation count is exact;
  c  the cap: at the trace's step count, one below it (the last iterate, clamped), and at 1;
  d  a workgroup's next system after one that ended as not finite, cap reached or converged;
  e  the warm start, of which only x > 0 is read;
  f  the two half-iteration routes at the block counts their tests skip.
Bounds: _assert_kkt and _assert_distance of tests/test_nnls_gpu.py, unchanged.  Why the cycling systems take exactly the
trace's steps in fp32 is tested without a GPU in tests/test_nnls.py (margin >= 2e-3 against a tolerance <= 7.7e-6).
"""
import numpy as np
import pytest
import torch

from tests import implicit_ref
from tests import nnls_ref as ref
from tests.test_nnls_gpu import (_assert_distance, _assert_kkt, _check_route, _dev, _explicit_systems, _mixed, _solve,
                                 _stats, _table)

pytestmark = pytest.mark.gpu

EDGE_FS = [15, 31, 47, 48, 63, 65, 79, 80, 95, 96, 111, 112, 127]
SCHEDULE_PAIRS = [p for p in ref.CYCLING_PAIRS if p != (72, 0)]
GRID = 2048  # kNnlsGrid: systems i and i + 2048 share a workgroup


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


@pytest.fixture(scope="module")
def cycling():
    """The fixture's cases with their fp64 traces, and which of them tell a run without Murty's rule apart."""
    fx = ref.load_cycling()
    A, b = fx["A"], fx["b"]
    traces = [ref.nnls_trace(a, v) for a, v in zip(A, b)]
    return A, b, traces, ref.cycling_needs_murty()


def _embed_all(A8, b8, f, o):
    out = [ref.embed(a, v, f, o) for a, v in zip(A8, b8)]
    return np.stack([e[0] for e in out]), np.stack([e[1] for e in out])


# ---------------------------------------------------------------------------------------------------------------------
# a. every instantiation at both edges
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f", EDGE_FS)
def test_nnls_block_count_edges(oracle, alslib, f):
    """The assertions of test_nnls_solve_batched, then again with A and b both scaled by 2^20 and 2^-20: x* is the same
    and both bounds are relative, so an absolute tolerance in the kernel would show."""
    rng = np.random.RandomState(1000 + f)
    batch = 64
    A1 = ref.random_spd(rng, batch, f)
    b1 = rng.standard_normal((batch, f)).astype(np.float32)
    for scale in (1.0, 2.0 ** 20, 2.0 ** -20):
        A, b = A1 * np.float32(scale), b1 * np.float32(scale)  # exact
        what = f"f={f} scale={scale:g}"
        A0, b0 = A.copy(), b.copy()
        x, st, Ag, bg = _solve(A, b, np.zeros_like(b))  # cold start
        _assert_kkt(A, b, x, "cold " + what)
        xs, Fs = _assert_distance(oracle, A, b, x, "cold " + what)
        assert st[0] == 0, (what, st)
        assert torch.equal(Ag.cpu(), torch.from_numpy(A0)) and torch.equal(bg.cpu(), torch.from_numpy(b0))  # not modified
        x2, st2, _, _ = _solve(A, b, np.zeros_like(b))
        assert np.array_equal(_bits(x), _bits(x2)) and np.array_equal(st, st2), what  # bit-identical runs
        # warm start from x*: one factorisation per system with a non-empty support
        xw, stw, _, _ = _solve(A, b, xs.astype(np.float32))
        _assert_kkt(A, b, xw, "warm " + what)
        _assert_distance(oracle, A, b, xw, "warm " + what)
        assert stw[0] == 0 and stw[1] == int(Fs.any(1).sum()), (what, stw, int(Fs.any(1).sum()))
        print(f"nnls {what}: cold {st[1] / batch:.2f} factorisations per system, warm {stw[1] / batch:.2f}")


# ---------------------------------------------------------------------------------------------------------------------
# b. the pivoting schedule, including the backup rule, against the trace
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f,o", SCHEDULE_PAIRS)
def test_nnls_schedule_follows_the_trace(oracle, alslib, cycling, f, o):
    """All cycling cases embedded at (f, o) in one batch from a cold start: converged, the factorisation count of the
    traces exactly, KKT, distance, and the trace's support.  A Murty step above the split flips 63 - clz(V1), below it
    63 - clz(V0); at o = 60 the block's indices 0..3 are below and 4..7 above.  A wrong index, a skipped backup step or
    a backup counter off by one changes the count (tests/test_nnls.py::test_cycling_cases_need_the_backup_rule).  The
    cases that tell a run without the rule apart are also solved one by one, for a count per case."""
    A8, b8, traces, needs = cycling
    A, b = _embed_all(A8, b8, f, o)
    emb = [ref.nnls_trace(a, v) for a, v in zip(A, b)]
    for k, (e, t) in enumerate(zip(emb, traces)):
        murty = [s.index for s in e.steps if s.murty]
        print(f"case {k} at f={f} o={o}: {len(e.steps)} steps, Murty flips {murty}, margin per step "
              + " ".join(f"{s.margin:.1e}" for s in e.steps))
        assert e.factorisations == t.factorisations and murty == [o + s.index for s in t.steps if s.murty]
    want = sum(e.factorisations for e in emb)
    x, st, _, _ = _solve(A, b, np.zeros_like(b))
    assert st[0] == 0, st
    assert st[1] == want, (st, want)
    _assert_kkt(A, b, x, f"cycling f={f} o={o}")
    _assert_distance(oracle, A, b, x, f"cycling f={f} o={o}")
    for k, e in enumerate(emb):
        assert np.array_equal(x[k] > 0, e.F & (e.x > 0)), (k, np.nonzero(x[k] > 0)[0], np.nonzero(e.F)[0])
    assert needs.sum() >= 10
    for k in np.nonzero(needs)[0]:
        xk, stk, _, _ = _solve(A[k:k + 1], b[k:k + 1], np.zeros_like(b[k:k + 1]))
        assert stk[0] == 0 and stk[1] == emb[k].factorisations, (k, stk, emb[k].factorisations)
        assert np.array_equal(_bits(xk[0]), _bits(x[k])), k


# ---------------------------------------------------------------------------------------------------------------------
# c. the cap
# ---------------------------------------------------------------------------------------------------------------------

def test_nnls_cap_at_the_step_count_and_one_below(oracle, alslib, cycling):
    """Each cycling case at (72, 60), n = its trace's step count.  max_iters = n converges with the bits of the default
    cap.  max_iters = n - 1 returns step n - 2's iterate, clamped: counted as not converged, the factorisations of
    steps 0..n-2, max(x_{n-2}, 0) on that step's passive set within the distance bound (yardstick: the fp32 oracle LU
    of that step's masked system) and exactly 0 off it.  max_iters = 1 returns the cold start's empty passive set."""
    A8, b8, _, _ = cycling
    f, o = 72, 60
    A, b = _embed_all(A8, b8, f, o)
    emb = [ref.nnls_trace(a, v) for a, v in zip(A, b)]
    x0, st0, _, _ = _solve(A, b, np.zeros_like(b))
    assert st0[0] == 0 and st0[1] == sum(e.factorisations for e in emb), st0
    # the yardstick of every case's step n - 2, in one oracle call
    last = [e.steps[-2] for e in emb]
    Am, bm = np.empty_like(A), np.empty_like(b)
    for k, s in enumerate(last):
        Am[k], bm[k] = ref.masked_system(A[k], b[k], s.F)
    x_lu = oracle.lu(Am, bm, f)
    for k, e in enumerate(emb):
        n = len(e.steps)
        assert n >= 3
        Ak, bk, zk = A[k:k + 1], b[k:k + 1], np.zeros_like(b[k:k + 1])
        xn, stn, _, _ = _solve(Ak, bk, zk, max_iters=n)
        assert stn[0] == 0 and stn[1] == e.factorisations, (k, n, stn)
        assert np.array_equal(_bits(xn[0]), _bits(x0[k])), (k, n)
        xc, stc, _, _ = _solve(Ak, bk, zk, max_iters=n - 1)
        s = last[k]
        facts = sum(bool(t.F.any()) for t in e.steps[:n - 1])
        assert stc[0] == 1 and stc[1] == facts, (k, n, stc, facts)
        assert not xc[0][~s.F].any() and (xc[0] >= 0).all(), (k, xc[0])
        e_o = np.abs(x_lu[k] - s.x).max()
        e_h = np.abs(xc[0] - np.maximum(s.x, 0)).max()
        bound = 2 * e_o + 1e-5 * np.abs(s.x).max()
        print(f"case {k}: n={n}, |x - x_(n-2)| {e_h:.2e}, oracle {e_o:.2e}, bound {bound:.2e}")
        assert e_h <= bound, (k, e_h, e_o)
        assert (s.x[s.F] < 0).any() or (s.y[~s.F] < 0).any()  # step n - 2 is not the solution
    x1, st1, _, _ = _solve(A, b, np.zeros_like(b), max_iters=1)
    assert not x1.any() and st1[0] == len(b) and st1[1] == 0, st1


# ---------------------------------------------------------------------------------------------------------------------
# d. state between systems of one workgroup
# ---------------------------------------------------------------------------------------------------------------------

POISON_KINDS = 6
SMALL_CAP = 4


def _poison(rng, A, A8, b8):
    """As many systems as the SPD matrices A, cycling through: NaN in b, NaN on the diagonal, a zero matrix with mixed-sign b, an all-positive
    solution with b > 0 (two steps: everything enters at once), b <= 0 (one step, no factorisation), a cycling case at
    o = 0 (more than SMALL_CAP steps).  Returns (A, b, kind)."""
    A = A.copy()
    n, f = A.shape[:2]
    b = rng.standard_normal((n, f)).astype(np.float32)
    kind = np.arange(n) % POISON_KINDS
    for i in range(n):
        if kind[i] == 0:
            b[i, (5 * i) % f] = np.nan
        elif kind[i] == 1:
            j = (7 * i) % f
            A[i, j, j] = np.nan
        elif kind[i] == 2:
            A[i] = 0
            b[i, 0], b[i, f - 1] = 1.0, -1.0
        elif kind[i] == 3:
            Z = np.abs(rng.standard_normal((f + 4, f)))
            P = (Z.T @ Z / (f + 4) + 0.1 * np.eye(f)).astype(np.float32)
            A[i] = 0.5 * (P + P.T)  # entries >= 0, so b = A x0 > 0 for x0 > 0
            b[i] = (A[i].astype(np.float64) @ rng.uniform(0.5, 2.0, f)).astype(np.float32)
        elif kind[i] == 4:
            b[i] = -np.abs(b[i])
        else:
            c = (i // POISON_KINDS) % len(b8)
            A[i], b[i] = ref.embed(A8[c], b8[c], f, 0)
    return A, b, kind


@pytest.mark.parametrize("f", [8, 72])
def test_nnls_workgroup_state_does_not_leak(alslib, cycling, f):
    """2048 good systems alone (A), after 2048 poison systems (B: system i + 2048 runs in poison system i's workgroup,
    right after it), and the poison alone (C), at the default cap and at one small enough that the cycling rows end as
    "cap reached": the good systems' bits do not depend on what their workgroup solved before, and the statistics
    add up."""
    A8, b8, traces, _ = cycling
    assert min(len(t.steps) for t in traces) > SMALL_CAP
    rng = np.random.RandomState(77 + f)
    Ag = np.tile(ref.random_spd(rng, GRID // 4, f), (4, 1, 1))  # 512 matrices, 2048 different right-hand sides
    bg = rng.standard_normal((GRID, f)).astype(np.float32)
    Ap, bp, kind = _poison(rng, Ag, A8, b8)
    Ab, bb = np.concatenate([Ap, Ag]), np.concatenate([bp, bg])
    for cap in (0, SMALL_CAP):
        xa, sa, _, _ = _solve(Ag, bg, np.zeros_like(bg), max_iters=cap)
        xb, sb, _, _ = _solve(Ab, bb, np.zeros_like(bb), max_iters=cap)
        xc, sc, _, _ = _solve(Ap, bp, np.zeros_like(bp), max_iters=cap)
        assert np.array_equal(_bits(xb[GRID:]), _bits(xa)), (f, cap, int((_bits(xb[GRID:]) != _bits(xa)).any(1).sum()))
        assert np.array_equal(_bits(xb[:GRID]), _bits(xc)), (f, cap)
        assert np.array_equal(sb, sa + sc), (f, cap, sa, sb, sc)
        hopeless = kind <= 2 if cap == 0 else (kind <= 2) | (kind == 5)  # kinds 3 and 4 take 2 steps and 1
        assert sc[0] == int(hopeless.sum()), (f, cap, sc, int(hopeless.sum()))
        assert not xc[kind <= 2].any(), (f, cap)
        assert not np.isnan(xc).any() and (xc >= 0).all(), (f, cap)
        if cap == 0:
            assert sa[0] == 0, sa
        ok = kind >= 3 if cap == 0 else (kind == 3) | (kind == 4)
        _assert_kkt(Ap[ok], bp[ok], xc[ok], f"converged poison rows f={f} cap={cap}")
        print(f"f={f} cap={cap}: stats good {sa.tolist()}, poison {sc.tolist()}, both {sb.tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# e. the warm start reads only x > 0
# ---------------------------------------------------------------------------------------------------------------------

def _warm(rng, p):
    """Two warm starts with the passive set p: 1 / 0, and any positive value / any value that is not > 0."""
    pos = np.array([np.float32(2.0 ** -149), 1e-30, 3.5, np.inf], np.float32)  # the smallest denormal first
    neg = np.array([0.0, -0.0, -2.0, -np.inf, np.nan], np.float32)
    w1 = np.where(p, np.float32(1), np.float32(0))
    w2 = np.where(p, pos[rng.randint(0, len(pos), p.shape)], neg[rng.randint(0, len(neg), p.shape)])
    assert np.array_equal(w2 > 0, p) and np.array_equal(w1 > 0, p)
    return w1, w2


@pytest.mark.parametrize("f", [63, 64, 65, 128])
def test_nnls_warm_start_reads_only_the_sign(alslib, f):
    rng = np.random.RandomState(300 + f)
    batch = 64
    A = ref.random_spd(rng, batch, f)
    b = rng.standard_normal((batch, f)).astype(np.float32)
    p = rng.randint(0, 2, (batch, f)).astype(bool)
    single = [j for j in (63, 64, f - 1) if j < f]
    for k, j in enumerate(single):  # one passive index on either side of the split, and the last
        p[k] = False
        p[k, j] = True
    p[len(single)] = True
    p[len(single) + 1] = False
    for name, w in zip(("ones", "mixed"), _warm(rng, p)):
        x, st, _, _ = _solve(A, b, w)
        _assert_kkt(A, b, x, f"warm start {name} f={f}")
        assert st[0] == 0, (name, st)
        if name == "ones":
            x1, st1 = x, st
    assert np.array_equal(_bits(x), _bits(x1)) and np.array_equal(st, st1), (f, st, st1)
    # systems that are solved by x = 0: b <= 0 from "none", b = 0 from "none" and from "all"
    none, every = np.zeros((batch, f), bool), np.ones((batch, f), bool)
    bn = -np.abs(b)
    bn[::3] = 0  # some exactly 0 entries too
    bz = np.zeros_like(b)
    for bb, pp, facts in ((bn, none, 0), (bz, none, 0), (bz, every, batch)):
        got = []
        for w in _warm(rng, pp):
            x, st, _, _ = _solve(A, bb, w)
            assert not x.any() and st[0] == 0 and st[1] == facts, (f, st, facts)
            got.append((_bits(x), st))
        assert np.array_equal(got[0][0], got[1][0])


# ---------------------------------------------------------------------------------------------------------------------
# f. the routes at the block counts their tests skip
# ---------------------------------------------------------------------------------------------------------------------

ROUTE_FS = [16, 48, 80, 112, 126]  # NB 2, 4, 6, 8, and the upper edge of 8 among the even f of the routes


@pytest.mark.parametrize("gram_mode", ["exact"], indirect=True)
@pytest.mark.parametrize("f", ROUTE_FS)
def test_update_nonneg_explicit_other_block_counts(oracle, alslib, gram_mode, f):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _mixed()
    Y = _table(f, 3)
    lam = 0.05
    A64, b64 = _explicit_systems(rowptr, colidx, val, Y, lam)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)  # warm start, mixed signs
    plan = als.Plan(rowptr, f)
    x, st = _dev(x0), _stats()
    als.update_nonneg(plan, _dev(colidx), _dev(val), _dev(Y), x, lam, stats=st)
    torch.cuda.synchronize()
    _check_route(oracle, lens, A64, b64, x.cpu().numpy(), f"explicit f={f} {gram_mode}")
    assert st[0].item() == 0, st
    plan.close()


@pytest.mark.parametrize("f", ROUTE_FS)
def test_update_nonneg_implicit_other_block_counts(oracle, alslib, f):
    from cumf_als_amd import als

    lens, rowptr, colidx, val = _mixed(11)
    val = (val - 2.0).astype(np.float32)  # negatives and stored zeros
    Y = _table(f, 5)
    lam, alpha, reg = 0.05, 40.0, "weighted"
    A64, b64 = implicit_ref.systems(rowptr, colidx, val, Y, lam, alpha, reg)
    x0 = (0.05 * np.random.RandomState(9).standard_normal((len(lens), f))).astype(np.float32)
    plan = als.Plan(rowptr, f)
    Yg = _dev(Y)
    x, st = _dev(x0), _stats()
    als.update_implicit_nonneg(plan, _dev(colidx), _dev(val), Yg, als.implicit_gram(Yg), x, lam, alpha, reg, stats=st)
    torch.cuda.synchronize()
    _check_route(oracle, lens, A64, b64, x.cpu().numpy(), f"implicit f={f} {reg}")
    assert st[0].item() == 0, st
    plan.close()
