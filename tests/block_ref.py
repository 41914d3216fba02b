"""numpy references of the block Gauss-Seidel solvers (als_block.h), shared by tests/test_block_ref.py and
tests/test_block_q_seams_gpu.py.

  block_dense      the recurrence on dense systems A x = b in the dtype of A: the oracle in fp64 (systems of tests/free_ref.py,
                   implicit_ref.py, weighted_ref.py, weighted_rank1_ref.py), an error-scale member in float32;
  block_sparse32   the recurrence as the kernels run it, in float32 throughout: a cached prediction per stored entry one block
                   step behind x, g and H summed one entry at a time in entry order, the Gram term apart.  An error scale, not
                   an oracle;
  row_error_scale  per row the largest distance to the fp64 recurrence over a family of float32 references: the dense recurrence
                   on the stored entry order and on seven fixed-seed orders, and block_sparse32 (with a Gram term in the
                   form of G x the row's kernel uses, on numpy's G and on G summed as the Gram kernels sum it:
                   gram_slabs).  The kernels are held to c x this, row by row, with no absolute floor.

Model bundles one model's data (the recipe of tests/test_block_explicit_gpu.py and its siblings), oracle and family.
"""
import functools

import numpy as np

from tests import free_ref, implicit_ref, nnls_ref, weighted_rank1_ref, weighted_ref

B = 32
C_ROW = 2.0  # the project's constant for these solvers
N_ORDERS = 7  # permuted dense members of the family; order N_ORDERS + 1 is held out (tests/test_block_ref.py)
LAM, W0 = 0.05, 0.25
KINDS = ("explicit", "nonneg", "implicit-weighted", "implicit-plain", "w0=0", "scalar", "rank1")


def _steps(f, sweeps):
    return [c for _ in range(sweeps) for c in range(0, f, B)]


def exact_step(H, rhs, xpi):
    return xpi + np.linalg.solve(H, rhs)


def solve_nopivot(H, rhs):
    """H d = rhs as block_solve32 eliminates it, in the dtype of H: no pivoting, the pivots' reciprocals multiplied."""
    H, rhs, n = H.copy(), rhs.copy(), len(rhs)
    rd = np.empty(n, H.dtype)
    for p in range(n):
        rd[p] = H.dtype.type(1) / H[p, p]
        l = H[p + 1:, p] * rd[p]
        H[p + 1:, p + 1:] -= l[:, None] * H[p, p + 1:]
        rhs[p + 1:] -= l * rhs[p]
    d = np.zeros(n, H.dtype)
    for p in reversed(range(n)):
        d[p] = rhs[p] * rd[p]
        rhs[:p] -= H[:p, p] * d[p]
    return d


def kernel_step(H, rhs, xpi):
    return xpi + solve_nopivot(H, rhs)


class NonnegStep:
    """The non-negative block step: the NNLS in z with c = rhs + H x[pi] from the passive set {x[pi] > 0} (fp64: the exact
    schedule; float32: the emulation of the solver's step, tests/nnls_ref.py).  `sets` records the passive set every call
    ends with, `eliminations` the factorisations."""

    def __init__(self):
        self.sets, self.eliminations = [], 0

    def __call__(self, H, rhs, xpi):
        solve = nnls_ref.nnls_trace_fp32 if H.dtype == np.float32 else nnls_ref.nnls_trace
        t = solve(H, rhs + H @ xpi, F0=xpi > 0)
        self.sets.append(t.x > 0)
        self.eliminations += t.factorisations
        return t.x


def block_dense(A, b, x0, sweeps, lens, step=exact_step):
    """`sweeps` sweeps of block Gauss-Seidel on A x = b from x0, in the dtype of A: x[pi] = step(A[pi, pi], (b - A x)[pi],
    x[pi]), the exact solve by default; rows without entries get 0."""
    x = x0.astype(A.dtype)
    for u in np.flatnonzero(np.asarray(lens) > 0):
        for c in _steps(x.shape[1], sweeps):
            x[u, c:c + B] = step(A[u, c:c + B, c:c + B], (b[u] - A[u] @ x[u])[c:c + B], x[u, c:c + B])
    x[np.asarray(lens) == 0] = 0
    return x


def entry_weight(kind, val, wgt=None, *, alpha=0.0, w0=0.0, own_e=None, gat_e=None, dtype=np.float32):
    """(w, c) of every stored entry as block_entry_weight forms them, in `dtype`: the entry adds w t t^T to H and
    t (c - w yhat) to g.  own_e, gat_e: the rank-one weights of the entry's row and column."""
    val = np.asarray(val, dtype)
    if kind == "none":
        return np.ones_like(val), val
    if kind == "alpha":
        w = dtype(alpha) * np.abs(val)
        return w, np.where(val > 0, 1 + w, 0).astype(dtype)
    wgt = np.asarray(wgt, dtype)
    if kind == "array":
        return wgt - dtype(w0), wgt * val
    if kind == "rank1":  # fma(-a_u, c_i, w): the product of two floats is exact in fp64
        return (wgt.astype(np.float64) - own_e.astype(np.float64) * gat_e.astype(np.float64)).astype(dtype), wgt * val
    raise ValueError(kind)


def _seq_sum(terms):
    """The sum over axis 0 one term at a time, in order, in the dtype of `terms`."""
    return np.cumsum(terms, axis=0, dtype=terms.dtype)[-1]


def _gram_pipe(G, x, c, bw):
    """(G x)[c : c + bw] as block_row_kernel forms it: K in steps of four, even and odd steps in two accumulators."""
    prod = x[:, None] * G[:, c:c + bw]
    even = (np.arange(len(x)) // 4) % 2 == 0
    acc0, acc1 = _seq_sum(prod[even]), (_seq_sum(prod[~even]) if (~even).any() else np.zeros(bw, prod.dtype))
    return acc0 + acc1


def block_sparse32(rowptr, colidx, val, Y, x0, lam, sweeps, *, weight=None, G=None, scale=None, reg="weighted",
                   step=kernel_step, gram="chain", dtype=np.float32, max_len=None):
    """The recurrence in the kernels' own form, float32 throughout.  Per row: yhat_e = t_e . x; per block step the step of the
    block before is folded into yhat, c_e - w_e yhat_e, g += t_e[pi] (c_e - w_e yhat_e) and H += w_e t_e[pi] t_e[pi]^T one entry
    at a time in entry order, reg on the diagonal, and with a Gram term H += s_u G[pi, pi] and
    rhs = (g - s_u (G x)[pi]) - reg x[pi]; then step(H, rhs, x[pi]), by default the elimination of block_solve32.
    reg: "weighted" or "plain", evaluated in fp32 as the kernels do, or one value per row.
    weight: None (w = 1, c = r) or the pair of entry_weight; G (f x f float32) with scale (one s_u per row; None: 1) is the
    Gram term; gram: "chain", u = G x as one chain over the columns, opened once and updated by every step
    (block_fused_gram_kernel), or "pipe", (G x)[pi] from x at every step (block_row_kernel).  dtype=np.float64 runs the same
    sums in fp64: the same recurrence as block_dense on the dense systems, which tests/test_block_ref.py checks.
    max_len: rows of more entries are not run and come back as nan."""
    Y = np.asarray(Y, dtype)
    f = Y.shape[1]
    w_all, c_all = (np.asarray(a, dtype) for a in (weight if weight is not None else entry_weight("none", val)))
    G = None if G is None else np.asarray(G, dtype)
    x = np.array(x0, dtype)
    for u in range(len(rowptr) - 1):
        s, e = int(rowptr[u]), int(rowptr[u + 1])
        if e == s or (max_len is not None and e - s > max_len):
            x[u] = 0 if e == s else np.nan
            continue
        T, w, c = Y[colidx[s:e]], w_all[s:e], c_all[s:e]
        rg = dtype(weighted_ref.reg_of(e - s, lam, reg) if isinstance(reg, str) else reg[u])
        su = dtype(1 if scale is None else scale[u])
        xu = x[u].copy()
        yhat = T @ xu
        if G is not None and gram == "chain":
            gx = _seq_sum(G * xu[:, None])
        prev = None
        for c0 in _steps(f, sweeps):
            bw = min(B, f - c0)
            if prev is not None:
                yhat = yhat + T[:, prev[0]:prev[0] + len(prev[1])] @ prev[1]
            Tp = T[:, c0:c0 + bw]
            g = _seq_sum(Tp * (c - w * yhat)[:, None])
            H = _seq_sum((w[:, None] * Tp)[:, :, None] * Tp[:, None, :])
            H[np.arange(bw), np.arange(bw)] += rg
            xpi = xu[c0:c0 + bw]
            if G is not None:
                H = H + su * G[c0:c0 + bw, c0:c0 + bw]
                g = g - su * (gx[c0:c0 + bw] if gram == "chain" else _gram_pipe(G, xu, c0, bw))
            new = step(H, g - rg * xpi, xpi).astype(dtype)
            prev = (c0, new - xpi)
            xu[c0:c0 + bw] = new
            if G is not None and gram == "chain":
                gx = gx + _seq_sum(G[c0:c0 + bw] * prev[1][:, None])
        x[u] = xu
    return x


_GRAMS = {}
# Members with G summed as the Gram kernels sum it, each on another order of the table's rows: N_GRAMS orders on every row and
# N_GRAMS_SHORT in all on the rows of at most SHORT_ROW entries; order N_GRAMS_SHORT is held out (tests/test_block_ref.py).  G's
# rounding error is the same for every row while a row's own matrix grows with its entries, so it is the short rows whose error
# is mostly G's and whose scale needs G sampled as often as the entry orders are; the long rows are also the costly ones here.
N_GRAMS, N_GRAMS_SHORT, SHORT_ROW = 3, 7, 128


def gram_slabs(Y, row_w=None, order=0):
    """G = Y^T diag(row_w) Y as implicit_gram / weighted_gram sum it (als_implicit.h): one float32 chain over the table rows of
    each slab (1024 rows up to f = 128, 1024 ceil(ceil(f / 16) / 8) above), the slabs' partials added in fp64.  Such a chain
    of some thousand terms rounds several times as much as a blocked float32 matrix product, and in a row of few entries
    G's error is most of the row's.  order > 0: the table rows in a fixed-seed random order (the same G, other roundings)."""
    key = (hash(Y.tobytes()), None if row_w is None else hash(row_w.tobytes()), order)
    if key not in _GRAMS:
        f = Y.shape[1]
        slab = 1024 * max(1, ((f + 15) // 16 + 7) // 8)
        perm = np.random.RandomState(3000 + order).permutation(len(Y)) if order else np.arange(len(Y))
        A = Y[perm] if row_w is None else Y[perm] * row_w[perm, None]
        G = np.zeros((f, f))
        for r0 in range(0, len(Y), slab):
            acc = np.zeros((f, f), np.float32)
            for n, r in enumerate(perm[r0:r0 + slab], r0):
                acc += A[n][:, None] * Y[r]
            G += acc
        _GRAMS[key] = G.astype(np.float32)
    return _GRAMS[key]


def reorder(rowptr, arrays, order):
    """`arrays` (one value per stored entry each) with the entries of every row in the fixed-seed random order `order`
    (0: as stored)."""
    if order == 0:
        return arrays
    rng = np.random.RandomState(1000 + order)
    perm = np.concatenate([s + rng.permutation(e - s) for s, e in zip(rowptr[:-1], rowptr[1:])]).astype(np.int64)
    return tuple(a[perm] for a in arrays)


class Model:
    """One model on the rows `lens`: the data, the fp64 oracle and the float32 family.
    kind: "explicit" | "nonneg" | "implicit-weighted" (alpha 1) | "implicit-plain" (alpha 40) | "w0=0" | "scalar" | "rank1"."""

    def __init__(self, kind, f, lens, n_cols, x0_seed=9):
        self.kind, self.f, self.lens = kind, f, list(lens)
        self.live = np.asarray(lens) > 0
        self.implicit, self.weighted = kind.startswith("implicit"), kind in ("w0=0", "scalar", "rank1")
        self.nonneg = kind == "nonneg"
        self.alpha, self.reg = (40.0, "plain") if kind == "implicit-plain" else (1.0, "weighted")
        self.w0 = W0 if kind == "scalar" else 0.0
        rng = np.random.RandomState(7)
        rows = len(lens)
        self.rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        self.colidx = np.concatenate([np.sort(rng.choice(n_cols, ln, replace=False)) for ln in lens]).astype(np.int32)
        nnz = int(self.rowptr[-1])
        ratings = [-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0] if self.implicit else [0.5, 1.0, 2.0, 3.0, 4.0, 5.0]
        self.val = rng.choice(np.array(ratings, np.float32), nnz)
        self.wgt = self.own = self.gat = None
        if self.weighted:
            self.wgt = rng.choice(np.array([0, 0.25, 0.5, 1.0, 2.0, 4.0], np.float32), nnz)
            if 17 in self.lens:  # a live row whose weights are all 0
                z = self.lens.index(17)
                self.wgt[self.rowptr[z]:self.rowptr[z + 1]] = 0
            self.own = (rng.uniform(0.1, 0.5, rows) * (rng.rand(rows) > 0.1)).astype(np.float32)
            gat = (rng.uniform(0.05, 1.0, n_cols) * (rng.rand(n_cols) > 0.1)).astype(np.float32)
            self.gat = (gat / gat.max()).astype(np.float32)  # the largest gather weight is exactly 1
        self.Y = (0.3 * np.random.RandomState(3).standard_normal((n_cols, f))).astype(np.float32)
        self.x0 = (0.05 * np.random.RandomState(x0_seed).standard_normal((rows, f))).astype(np.float32)

    def entries(self, order=0):
        """(colidx, val, wgt) in entry order `order`."""
        wgt = self.wgt if self.weighted else self.val
        return reorder(self.rowptr, (self.colidx, self.val, wgt), order)

    def systems(self, dtype, order=0):
        """The dense systems in `dtype` from the entries in order `order`.  With a Gram term the rows of the gathered table are
        reordered too (the same systems: the column indices follow), so that G = Y^T Y is summed in another order as well:
        in a short row G's rounding error is the whole error, and the entries' order alone would not sample it."""
        colidx, val, wgt = self.entries(order)
        Y, gat = self.Y, self.gat
        if order and self.has_gram:
            perm = np.random.RandomState(2000 + order).permutation(len(Y))
            Y, colidx = Y[perm], np.argsort(perm)[colidx]
            gat = gat[perm] if gat is not None else None
        if self.implicit:
            return implicit_ref.systems(self.rowptr, colidx, val, Y, LAM, self.alpha, self.reg, dtype=dtype)
        if self.kind == "rank1":
            return weighted_rank1_ref.systems(self.rowptr, colidx, val, wgt, Y, LAM, self.own, gat, self.reg, dtype)
        if self.weighted:
            return weighted_ref.systems(self.rowptr, colidx, val, wgt, Y, LAM, self.w0, self.reg, dtype)
        return free_ref.systems(self.rowptr, colidx, val, Y, LAM, dtype)

    def _run(self, fn, *args, **kw):
        """(x, the passive sets of every block step or None)."""
        if not self.nonneg:
            return fn(*args, **kw), None
        step = NonnegStep()
        return fn(*args, step=step, **kw), step.sets

    def dense(self, dtype, sweeps, order=0):
        A, b = self.systems(dtype, order)
        return self._run(block_dense, A, b, self.x0, sweeps, self.lens)

    def sparse32(self, sweeps, gram="chain", dtype=np.float32, slabs=None, max_len=None):
        """block_sparse32 on the model; `gram` matters where the model has a Gram term, and `slabs` (an order of gram_slabs)
        replaces numpy's G by one summed as the Gram kernels sum it."""
        Y = self.Y.astype(dtype)
        kw = {"reg": self.reg, "dtype": dtype, "gram": gram, "max_len": max_len}
        if self.implicit:
            kw.update(weight=entry_weight("alpha", self.val, alpha=self.alpha, dtype=dtype), G=Y.T @ Y)
            if dtype == np.float64:  # the implicit oracle's reg is the fp64 product
                kw["reg"] = [implicit_ref.reg_of(n, LAM, self.reg) for n in self.lens]
        elif self.kind == "rank1":
            row = np.repeat(np.arange(len(self.lens)), self.lens)
            kw.update(weight=entry_weight("rank1", self.val, self.wgt, own_e=self.own[row], gat_e=self.gat[self.colidx],
                                          dtype=dtype), G=(Y * self.gat[:, None].astype(dtype)).T @ Y, scale=self.own)
        elif self.weighted:
            kw.update(weight=entry_weight("array", self.val, self.wgt, w0=self.w0, dtype=dtype))
            if self.w0 > 0:
                kw.update(G=Y.T @ Y, scale=np.full(len(self.lens), self.w0, np.float32))
        if slabs is not None and "G" in kw:
            kw["G"] = gram_slabs(self.Y, self.gat if self.kind == "rank1" else None, slabs)
        return self._run(block_sparse32, self.rowptr, self.colidx, self.val, self.Y, self.x0, LAM, sweeps, **kw)

    @property
    def has_gram(self):
        return self.implicit or self.kind in ("scalar", "rank1")

    @functools.lru_cache(maxsize=None)
    def oracle(self, sweeps):
        """(x, passive sets) of the fp64 dense recurrence."""
        return self.dense(np.float64, sweeps)

    @functools.lru_cache(maxsize=None)
    def dense_members(self, sweeps):
        return [(f"dense32/{o}", *self.dense(np.float32, sweeps, o)) for o in range(N_ORDERS + 1)]

    def members(self, sweeps, gram="chain"):
        """The family: (name, x, passive sets) of every float32 reference.  A model with a Gram term has one family per form
        of G x: "chain" for the rows block_fused_gram_kernel takes, "pipe" for those block_row_kernel takes."""
        if not self.has_gram:
            return self.dense_members(sweeps) + [("sparse32", *self.sparse32(sweeps))]
        return self.dense_members(sweeps) + [(f"sparse32/{gram}", *self.sparse32(sweeps, gram))] + [
            (f"sparse32/{gram}/slabs{o}", *self.sparse32(sweeps, gram, slabs=o, max_len=None if o < N_GRAMS else SHORT_ROW))
            for o in range(N_GRAMS_SHORT)]

    def jumped(self, sets, sweeps):
        """Per row: a passive set of `sets` differs from the oracle's at some block step (non-negative model only)."""
        out = np.zeros(len(self.lens), bool)
        if sets is not None:
            per_row = len(_steps(self.f, sweeps))
            for n, u in enumerate(np.flatnonzero(self.live)):
                pairs = zip(sets[n * per_row:(n + 1) * per_row], self.oracle(sweeps)[1][n * per_row:(n + 1) * per_row])
                out[u] = any(not np.array_equal(a, b) for a, b in pairs)
        return out


def row_distance(x, x64):
    return np.abs(x - x64).max(1)


@functools.lru_cache(maxsize=None)
def row_error_scale(model, sweeps, gram="chain"):
    """(E, left_out, x32): E[u] the largest max-norm distance of a family member to the fp64 recurrence in row u; left_out[u]:
    some member's passive sets differ from the oracle's in row u, a jump and not rounding (non-negative model; E[u] then
    counts only the members that did not jump); x32: the dense float32 recurrence on the stored order, the scale of the
    pooled bound of the models' own test files."""
    x64 = model.oracle(sweeps)[0]
    E, left_out = np.zeros(len(model.lens)), np.zeros(len(model.lens), bool)
    for _, x, sets in model.members(sweeps, gram):
        jumped = model.jumped(sets, sweeps)
        d = row_distance(x, x64)  # nan: the member does not run that row
        E = np.maximum(E, np.where(jumped | np.isnan(d), 0, d))
        left_out |= jumped
    return E, left_out, model.dense_members(sweeps)[0][1]


def row_ratios(tag, x, model, sweeps, chain_rows=None):
    """Prints every live row's |x - x64|_max / E and returns (ratio, use), one per row: use[u], the row is live and held to the
    per-row bound (not left out of it); ratio is 0 elsewhere.  x must be finite, and exactly 0 in the rows without entries.  A
    row whose error is 0 has ratio 0 whatever E is, one with an error and E = 0 has inf.  chain_rows[u]: row u ran with G x as
    a chain (models with a Gram term; default: none did)."""
    x64 = model.oracle(sweeps)[0]
    E, left_out, _ = row_error_scale(model, sweeps, "pipe")
    if chain_rows is not None and model.has_gram and np.any(chain_rows):
        Ec, lc, _ = row_error_scale(model, sweeps, "chain")
        E, left_out = np.where(chain_rows, Ec, E), np.where(chain_rows, lc, left_out)
    assert np.isfinite(x).all(), (tag, np.flatnonzero(~np.isfinite(x).all(1)).tolist())
    assert (x[~model.live] == 0).all(), tag
    use = model.live & ~left_out
    err = np.where(use, row_distance(x, x64), 0)
    with np.errstate(divide="ignore"):
        ratio = np.divide(err, E, out=np.zeros(len(E)), where=err > 0)
    print(f"{tag}: " + " ".join(f"n={n}:{'left-out' if lo else format(r, '.3f')}"
                                for n, r, lo, lv in zip(model.lens, ratio, left_out, model.live) if lv)
          + f" | max {ratio[use].max() if use.any() else 0:.3f}")
    return ratio, use
