"""Multi-GPU implicit-feedback ALS: the confidence-weighted model of `als.ImplicitALSEngine` (Hu, Koren, Volinsky 2008;
include/cumf_implicit_capi.h) over the partitions and collectives of `cumf_als_amd.dist` -- one process per GPU,
`torch.distributed`, contiguous cost-balanced row slabs fixed for the run.

One side's systems are A_u = G + sum_i w_ui y_i y_i^T + reg_u I, b_u = sum_{r > 0} (1 + w_ui) y_i with G = Y^T Y over the
whole fixed table.  Two schemes, as in `dist.DistALS`:

* ``"gather"`` -- both tables replicated.  Every rank forms G of the full fixed table itself (the same bits in, a
  deterministic kernel: the same G everywhere), runs `update_implicit` on its slab's plan and the slabs are exchanged with
  ONE all-gather per half-iteration.  Nothing but factor rows leaves a GPU.
* ``"reduce"`` -- X row-sharded and device-resident, Theta replicated.  update-X: G of Theta locally, `update_implicit` on
  the slab, no communication.  update-Theta, per Theta batch: every rank forms the PARTIAL systems of the batch over its
  own X slab (`cumf_get_hermitian_implicit_partial`: packed upper triangles of sum w y y^T with lambda * n_local on the
  diagonal, and the right-hand sides), one reduce-scatter sums them and leaves each rank 1 / world of the systems;
  G_X = X^T X is the all-reduced sum of the slabs' Grams (once per half-iteration); `cumf_implicit_finish` adds it, the
  batched LU or CG solves, one all-gather returns Theta.  The Theta side issues its collectives one after the other: no
  communication runs under a kernel yet.

Compute is injected through an "ops" object as in `dist.DistALS`: the product ops are `HipImplicitOps` (libALS.so); the
CPU tests drive the same partition and collective code with a numpy stand-in.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from .dist import HostMatrix  # noqa: F401  (the matrix type the constructor takes, re-exported for callers)
from .dist import (SlabGather, all_gather_equal, all_gather_rows, balanced_slabs, local_csc_of_slab,
                   local_csc_of_slab_torch, reduce_scatter_rows, slice_csr, solve_row_cost)

_SOLVERS = ("cg", "lu", "cg_matfree")


class HipImplicitOps:
    """Compute ops backed by libALS.so on the current CUDA device."""

    dtype = torch.float32

    def __init__(self, device):
        from . import als

        self.als = als
        self.device = torch.device(device)

    def to_device(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def available(self, f: int, solver) -> bool:
        return self.als.implicit_available(f, solver)

    def plan(self, rowptr: np.ndarray, f: int, chunk: int = 0, row_begin: int = 0, row_end=None):
        return self.als.Plan(np.ascontiguousarray(rowptr), f, row_begin, row_end, chunk)

    def gram(self, table, G):
        self.als.implicit_gram(table, G)

    def update_implicit(self, plan, colidx, val, gather, G, update, lam, alpha, reg, solver, cg_iters):
        self.als.update_implicit(plan, colidx, val, gather, G, update, lam, alpha, reg, solver, cg_iters)

    def hermitian_partial(self, plan, colidx, val, gather, lam, alpha, reg, packed, rhs):
        self.als.get_hermitian_implicit_partial(plan, colidx, val, gather, lam, alpha, reg, packed, rhs)

    def finish(self, packed, G, reg_add, tt):
        self.als.implicit_finish(packed, G, reg_add, tt)

    def solve(self, tt, rhs, x, solver, cg_iters):
        if solver == "cg":
            self.als.cg_solve(tt, x, rhs, cg_iters)
        else:
            self.als.lu_solve(tt, rhs, x)

    def loss(self, rowptr, colidx, val, XT, thetaT, lam, alpha, reg) -> float:
        return float(self.als.implicit_loss(rowptr, colidx, val, XT, thetaT, lam, alpha, reg).item())

    def release_scratch(self) -> None:
        self.als.release_scratch()


def _solver_name(solver) -> str:
    names = {0: "cg", 1: "lu", 2: "cg_matfree", "CG": "cg", "LU": "lu"}
    solver = names.get(solver, solver)
    if solver not in _SOLVERS:
        raise ValueError(f"unknown solver {solver!r} (cg | lu | cg_matfree)")
    return solver


def _reg_name(reg) -> str:
    names = {0: "weighted", 1: "plain"}
    reg = names.get(reg, reg)
    if reg not in ("weighted", "plain"):
        raise ValueError(f"unknown reg mode {reg!r} (weighted | plain)")
    return reg


class DistImplicitALS:
    """Implicit-feedback ALS over `world` ranks.  Every rank constructs it with the same host matrix (or, for
    `scheme="reduce"`, its own row slab -- see `from_local_slab`).  solver "cg", "lu" (even 8 <= f <= 128) or
    "cg_matfree" (even 8 <= f <= 512); `solver_x` / `solver_theta` choose per side.  The Theta side of the `reduce` scheme
    solves materialised systems, so it takes "cg" and "lu" only."""

    def __init__(self, mat: HostMatrix, f: int, lam: float, alpha: float, ops, solver="cg", cg_iters: int = 3,
                 reg="weighted", scheme: str = "gather", theta_batch: int = 1, group=None, chunk: int = 0, solver_x=None,
                 solver_theta=None, cg_iters_x=None, cg_iters_theta=None):
        self._configure(f, lam, alpha, ops, solver, cg_iters, reg, scheme, theta_batch, group, solver_x, solver_theta,
                        cg_iters_x, cg_iters_theta)
        self.m, self.n = mat.m, mat.n
        self._mat = mat
        dev = self._device()
        self.thetaT = torch.zeros((self.n, f), dtype=ops.dtype, device=dev)
        self.xb = balanced_slabs(mat.csr_indptr, self.world, solve_row_cost(f, self.solver_x))
        x0, x1 = int(self.xb[self.rank]), int(self.xb[self.rank + 1])
        rp, ci, va = slice_csr(mat.csr_indptr, mat.csr_indices, mat.csr_data, x0, x1)
        self._set_x_slab(np.asarray(rp), ops.to_device(ci), ops.to_device(va), chunk)
        if scheme == "gather":
            self.XT = torch.zeros((self.m, f), dtype=ops.dtype, device=dev)
            self.tb = balanced_slabs(mat.csc_indptr, self.world, solve_row_cost(f, self.solver_theta))
            t0, t1 = int(self.tb[self.rank]), int(self.tb[self.rank + 1])
            rp, ci, va = slice_csr(mat.csc_indptr, mat.csc_indices, mat.csc_data, t0, t1)
            self.t_plan = ops.plan(np.asarray(rp), f, chunk)
            self.t_colidx, self.t_val = ops.to_device(ci), ops.to_device(va)
            self._gx = SlabGather(self.xb, f, ops.dtype, dev, group)
            self._gt = SlabGather(self.tb, f, ops.dtype, dev, group)
            self._full_csr = None  # the whole CSR on the device, uploaded by the first loss()
        else:
            self.XT = torch.zeros((self.x_rows, f), dtype=ops.dtype, device=dev)
            cp, ri, cv = local_csc_of_slab(np.asarray(rp), np.asarray(ci), np.asarray(va), self.n)
            self._set_theta_batches(np.asarray(cp, dtype=np.int64), ops.to_device(ri), ops.to_device(cv), chunk)

    @classmethod
    def from_local_slab(cls, m_total: int, n: int, xb, rowptr_l: torch.Tensor, colidx_l: torch.Tensor, val_l: torch.Tensor,
                        f: int, lam: float, alpha: float, ops, solver="cg", cg_iters: int = 3, reg="weighted",
                        theta_batch: int = 1, group=None, chunk: int = 0, solver_x=None, solver_theta=None,
                        cg_iters_x=None, cg_iters_theta=None) -> "DistImplicitALS":
        """`reduce` scheme from this rank's row slab only (no rank ever holds the whole matrix).  `xb`: the world + 1
        global slab boundaries; the three tensors are the slab's CSR with the row pointer rebased to 0, already on the
        device."""
        self = cls.__new__(cls)
        self._configure(f, lam, alpha, ops, solver, cg_iters, reg, "reduce", theta_batch, group, solver_x, solver_theta,
                        cg_iters_x, cg_iters_theta)
        self.m, self.n = m_total, n
        self._mat = None
        self.xb = np.asarray(xb, dtype=np.int64)
        dev = colidx_l.device
        self.thetaT = torch.zeros((n, f), dtype=ops.dtype, device=dev)
        self._set_x_slab(rowptr_l.cpu().numpy(), colidx_l, val_l, chunk)
        self.XT = torch.zeros((self.x_rows, f), dtype=ops.dtype, device=dev)
        cp, ri, cv = local_csc_of_slab_torch(rowptr_l, colidx_l, val_l, n)
        self._set_theta_batches(np.asarray(cp, dtype=np.int64), ri, cv, chunk)
        return self

    # -- construction ------------------------------------------------------------------------
    def _configure(self, f, lam, alpha, ops, solver, cg_iters, reg, scheme, theta_batch, group, solver_x, solver_theta,
                   cg_iters_x, cg_iters_theta) -> None:
        if scheme not in ("gather", "reduce"):
            raise ValueError(f"unknown scheme {scheme!r} (gather | reduce)")
        self.f, self.lam, self.alpha, self.ops = int(f), float(lam), float(alpha), ops
        self.reg, self.scheme, self.theta_batch, self.group = _reg_name(reg), scheme, int(theta_batch), group
        self.solver, self.cg_iters = _solver_name(solver), int(cg_iters)
        self.solver_x = self.solver if solver_x is None else _solver_name(solver_x)
        self.solver_theta = self.solver if solver_theta is None else _solver_name(solver_theta)
        self.cg_iters_x = self.cg_iters if cg_iters_x is None else int(cg_iters_x)
        self.cg_iters_theta = self.cg_iters if cg_iters_theta is None else int(cg_iters_theta)
        if scheme == "reduce" and self.solver_theta == "cg_matfree":
            raise ValueError("scheme 'reduce' solves the Theta side from reduced, materialised systems: solver_theta must "
                             "be 'lu' or 'cg' ('cg_matfree' forms no system; it may still be chosen with solver_x)")
        available = getattr(ops, "available", None)
        for side, s in (("x", self.solver_x), ("theta", self.solver_theta)):
            if available is not None and not available(self.f, s):
                raise ValueError(f"implicit ALS takes even 8 <= f <= 128 with solver cg | lu and even 8 <= f <= 512 with "
                                 f"cg_matfree (got f = {f}, solver_{side} = {s!r})")
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1

    def _device(self):
        return self.ops.to_device(np.zeros(1, np.float32)).device

    def _set_x_slab(self, rowptr_l: np.ndarray, colidx, val, chunk: int) -> None:
        self.x_rows = len(rowptr_l) - 1
        self.x_plan = self.ops.plan(rowptr_l, self.f, chunk)
        self.x_rowptr_host = rowptr_l
        self.x_colidx, self.x_val = colidx, val
        self.G = torch.empty((self.f, self.f), dtype=self.ops.dtype, device=colidx.device)
        self.t_plan = None
        self.t_batches = []

    def _set_theta_batches(self, cp: np.ndarray, rowidx, val, chunk: int) -> None:
        """`reduce` scheme: the slab-local CSC, the Theta batches' plans over it, the columns without an entry on any rank
        and the communication buffers (built once; nothing is allocated per half-iteration)."""
        f, w, dev, dtype = self.f, self.world, self.thetaT.device, self.ops.dtype
        self.lc_rowidx, self.lc_val = rowidx, val
        cnt = torch.from_numpy(np.diff(cp).astype(np.int64))  # stored entries of this slab per Theta column
        self._all_reduce(cnt)                                 # ... and of all slabs: the one integer all-reduce
        self._t_empty = torch.nonzero(cnt == 0).reshape(-1).to(dev)
        n = self.n
        for b in range(self.theta_batch):
            size = n // self.theta_batch if b != self.theta_batch - 1 else n - b * (n // self.theta_batch)
            off = b * (n // self.theta_batch)
            self.t_batches.append((off, size, self.ops.plan(cp, f, chunk, off, off + size)))
        kmax = max((size + w - 1) // w for (_, size, _) in self.t_batches)
        pk = f * (f + 1) // 2
        self._tri = torch.zeros((w * kmax, pk), dtype=dtype, device=dev)
        self._rhs = torch.zeros((w * kmax, f), dtype=dtype, device=dev)
        self._mine = torch.empty((kmax, pk), dtype=dtype, device=dev)
        self._mine_rhs = torch.empty((kmax, f), dtype=dtype, device=dev)
        self._my_tt = torch.empty((kmax, f, f), dtype=dtype, device=dev)
        self._x = torch.zeros((kmax, f), dtype=dtype, device=dev)
        self._gathered = torch.empty((w * kmax, f), dtype=dtype, device=dev)
        self._x_rowptr32 = None  # the slab's row pointer on the device (int32), uploaded by the first loss()

    def _all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        """Sum `t` over the ranks in place (through the host when the backend cannot take the tensor where it lives)."""
        if not dist.is_initialized() or self.world == 1:
            return t
        nccl = dist.get_backend(self.group) == "nccl"
        if t.is_cuda == nccl:
            dist.all_reduce(t, group=self.group)
        else:
            buf = t.to(self.thetaT.device) if nccl else t.cpu()
            dist.all_reduce(buf, group=self.group)
            t.copy_(buf)
        return t

    # -- factors -----------------------------------------------------------------------------
    def init_factors(self, thetaT: np.ndarray, XT: np.ndarray | None = None) -> None:
        self.thetaT.copy_(torch.from_numpy(np.ascontiguousarray(thetaT)).reshape(self.n, self.f))
        if XT is None:
            self.XT.zero_()
        else:
            XT = np.ascontiguousarray(XT).reshape(self.m, self.f)
            if self.scheme == "reduce":
                XT = XT[int(self.xb[self.rank]):int(self.xb[self.rank + 1])]
            self.XT.copy_(torch.from_numpy(np.ascontiguousarray(XT)))

    def full_XT(self) -> torch.Tensor:
        """X on every rank (gathers the slabs in the "reduce" scheme)."""
        if self.scheme == "gather":
            return self.XT
        out = torch.empty((self.m, self.f), dtype=self.XT.dtype, device=self.XT.device)
        if dist.is_initialized():
            all_gather_rows(out, self.XT, self.xb, self.group)
        else:
            out.copy_(self.XT)
        return out

    # -- half-iterations ---------------------------------------------------------------------
    def _update_slab(self, plan, colidx, val, table, out, bounds, gather_all, solver, cg_iters) -> None:
        """`gather` scheme, one side: G of the replicated `table`, this rank's slab of `out`, the slabs exchanged."""
        self.ops.gram(table, self.G)
        mine = out[int(bounds[self.rank]):int(bounds[self.rank + 1])]
        self.ops.update_implicit(plan, colidx, val, table, self.G, mine, self.lam, self.alpha, self.reg, solver, cg_iters)
        gather_all(out, mine)

    def update_x(self) -> None:
        if self.scheme == "gather":
            self._update_slab(self.x_plan, self.x_colidx, self.x_val, self.thetaT, self.XT, self.xb, self._gx,
                              self.solver_x, self.cg_iters_x)
        else:
            self.ops.gram(self.thetaT, self.G)
            self.ops.update_implicit(self.x_plan, self.x_colidx, self.x_val, self.thetaT, self.G, self.XT, self.lam,
                                     self.alpha, self.reg, self.solver_x, self.cg_iters_x)

    def update_theta(self) -> None:
        if self.scheme == "gather":
            self._update_slab(self.t_plan, self.t_colidx, self.t_val, self.XT, self.thetaT, self.tb, self._gt,
                              self.solver_theta, self.cg_iters_theta)
            return
        w = self.world
        # G_X = X^T X: the sum over the ranks of the Grams of their slabs, once per half-iteration
        self.ops.gram(self.XT, self.G)
        self._all_reduce(self.G)
        reg_add = self.lam if self.reg == "plain" else 0.0  # weighted: the partials carry lambda * n_local already
        for off, size, plan in self.t_batches:
            k = (size + w - 1) // w
            tri, rhs = self._tri[: w * k], self._rhs[: w * k]
            self.ops.hermitian_partial(plan, self.lc_rowidx, self.lc_val, self.XT, self.lam, self.alpha, self.reg,
                                       tri[:size], rhs[:size])
            if size < w * k:  # the padding systems behind the last rank's share
                tri[size:].zero_()
                rhs[size:].zero_()
            reduce_scatter_rows(tri, self.group, out=self._mine[:k])
            reduce_scatter_rows(rhs, self.group, out=self._mine_rhs[:k])
            lo, hi = min(self.rank * k, size), min((self.rank + 1) * k, size)
            x = self._x[:k]
            if hi > lo:
                self.ops.finish(self._mine[: hi - lo], self.G, reg_add, self._my_tt[: hi - lo])
                x[: hi - lo].copy_(self.thetaT[off + lo: off + hi])  # CG warm start
                self.ops.solve(self._my_tt[: hi - lo], self._mine_rhs[: hi - lo], x[: hi - lo], self.solver_theta,
                               self.cg_iters_theta)
            gathered = self._gathered[: w * k]
            all_gather_equal(gathered, x, self.group)
            self.thetaT[off: off + size].copy_(gathered[:size])
        if self._t_empty.numel():  # columns without an entry on any rank: exactly 0, as the single-GPU engine leaves them
            self.thetaT.index_fill_(0, self._t_empty, 0.0)

    def iterate(self, iters: int = 1) -> None:
        for _ in range(iters):
            self.update_x()
            self.update_theta()

    # -- the objective -----------------------------------------------------------------------
    def loss(self) -> float:
        """The implicit objective of the current factors (fp64), the same value on every rank.  `reduce` scheme: every rank
        evaluates it on its slab (X slab, slab CSR, full Theta) and the values are summed -- the Frobenius term is linear
        in X^T X, the stored-entry terms and the weighted regulariser are sums over entries; the plain regulariser's
        lambda tr(Theta^T Theta) is then counted once per rank, so (world - 1) times it is taken off again."""
        ops = self.ops
        if self.scheme == "gather":
            if self._full_csr is None:
                m = self._mat
                self._full_csr = (ops.to_device(np.asarray(m.csr_indptr).astype(np.int32)), ops.to_device(m.csr_indices),
                                  ops.to_device(m.csr_data))
            rp, ci, va = self._full_csr
            return ops.loss(rp, ci, va, self.XT, self.thetaT, self.lam, self.alpha, self.reg)
        if self._x_rowptr32 is None:
            self._x_rowptr32 = ops.to_device(np.asarray(self.x_rowptr_host).astype(np.int32))
        mine = ops.loss(self._x_rowptr32, self.x_colidx, self.x_val, self.XT, self.thetaT, self.lam, self.alpha, self.reg)
        total = float(self._all_reduce(torch.tensor([mine], dtype=torch.float64)).item())
        if self.reg == "plain" and self.world > 1:
            total -= (self.world - 1) * self.lam * float((self.thetaT.double() ** 2).sum().item())
        return total

    def close(self) -> None:
        """Destroy the plans and hand the library's pooled scratch of this device back."""
        for p in [getattr(self, "x_plan", None), getattr(self, "t_plan", None)] + [p for (_, _, p) in self.t_batches]:
            if p is not None and hasattr(p, "close"):
                p.close()
        self.x_plan = self.t_plan = None
        self.t_batches = []
        release = getattr(self.ops, "release_scratch", None)
        if release is not None:
            release()
