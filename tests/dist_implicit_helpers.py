"""What tests/test_dist_implicit_cpu.py and tests/test_dist_implicit_gpu.py share: the data set, a numpy stand-in for the
compute ops of cumf_als_amd.dist_implicit, a single-process fp64 implicit ALS, and the entry point of a spawned rank.

TEST INFRASTRUCTURE: the product's ops are `cumf_als_amd.dist_implicit.HipImplicitOps` (HIP kernels).  The CPU tier has no
GPU, so the partition + collective logic of DistImplicitALS runs there with numpy doing the per-rank arithmetic, in fp64 so
that the only differences from the single-process run are summation orders.  Never imported by the package.
"""
import numpy as np
import torch

from tests import implicit_ref as ref

EMPTY_COL = 17  # no entry at all: its Theta row must stay exactly 0
LOCAL_COL = 41  # entries only in the first LOCAL_ROWS rows: all in rank 0's slab
LOCAL_ROWS = 12
VALUES = np.array([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0, 5.0], np.float32)  # negatives and stored zeros


def make_data(m=120, n=90, nnz=6000, seed=12):
    """CSR + CSC (the fields of dist.HostMatrix) of an m x n matrix with exactly nnz stored entries, rows of very unequal
    length, column EMPTY_COL empty and column LOCAL_COL stored in rows < LOCAL_ROWS only."""
    rng = np.random.RandomState(seed)
    weight = np.outer(1.0 / (1.0 + np.arange(m)) ** 0.35, 0.3 + rng.random_sample(n))
    weight[:, EMPTY_COL] = 0.0
    weight[LOCAL_ROWS:, LOCAL_COL] = 0.0
    weight[:LOCAL_ROWS, LOCAL_COL] *= 50.0
    key = rng.random_sample((m, n)) ** (1.0 / np.maximum(weight, 1e-300))  # weighted sampling without replacement
    key[weight == 0.0] = -1.0
    cells = np.argsort(-key, axis=None)[:nnz]
    mask = np.zeros((m, n), bool)
    mask.flat[cells] = True
    R = np.zeros((m, n), np.float32)
    R[mask] = rng.choice(VALUES, nnz)
    row, col = np.nonzero(mask)             # row-major: CSR order
    colT, rowT = np.nonzero(mask.T)         # column-major: CSC order
    d = {"csr_indptr": np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32),
         "csr_indices": col.astype(np.int32), "csr_data": R[row, col],
         "csc_indptr": np.concatenate([[0], np.cumsum(mask.sum(0))]).astype(np.int32),
         "csc_indices": rowT.astype(np.int32), "csc_data": R[rowT, colT]}
    assert d["csr_indptr"][-1] == nnz and (d["csr_data"] < 0).any()
    return d


def stored_dense(d, m, n):
    """m x n array of the stored values, NaN where nothing is stored (implicit_ref.dense_loss)."""
    R = np.full((m, n), np.nan)
    rows = np.repeat(np.arange(m), np.diff(d["csr_indptr"]))
    R[rows, d["csr_indices"]] = d["csr_data"]
    return R


def cg(A, x0, b, iters):
    """The recurrence of cumf_cg_solve_batched on a batch, in the dtype of A: warm start, at most `iters` steps, a
    system stops once r.r < 1e-4."""
    x = np.array(x0, A.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(len(A)):
            r = b[s] - A[s] @ x[s]
            p = r.copy()
            rsold = r @ r
            for _ in range(iters):
                ap = A[s] @ p
                a = rsold / (p @ ap)
                x[s] += a * p
                r -= a * ap
                rsnew = r @ r
                if rsnew < 1e-4:
                    break
                p = r + (rsnew / rsold) * p
                rsold = rsnew
    return x


def solve(A, b, x0, solver, iters):
    return cg(A, x0, b, iters) if solver == "cg" else np.linalg.solve(A, b[..., None])[..., 0]


def als_fp64(d, m, n, f, lam, alpha, reg, solver, cg_iters, iters, theta0):
    """Single-process implicit ALS in fp64 on the systems of tests/implicit_ref.py: (thetaT, XT)."""
    th, x = np.asarray(theta0, np.float64).copy(), np.zeros((m, f))

    def half(rowptr, colidx, val, Y, out):
        A, b = ref.systems(rowptr, colidx, val, Y, lam, alpha, reg)
        empty = np.diff(rowptr) == 0
        A[empty] = np.eye(f)
        new = solve(A, b, out, solver, cg_iters)
        new[empty] = 0.0
        return new

    for _ in range(iters):
        x = half(d["csr_indptr"], d["csr_indices"], d["csr_data"], th, x)
        th = half(d["csc_indptr"], d["csc_indices"], d["csc_data"], x, th)
    return th, x


class _Plan:
    def __init__(self, rowptr, f, row_begin, row_end):
        self.rowptr = np.ascontiguousarray(rowptr).astype(np.int64)
        self.f = f
        self.row_begin = row_begin
        self.row_end = len(rowptr) - 1 if row_end is None else row_end


class NumpyImplicitOps:
    """Stand-in of HipImplicitOps on CPU tensors; `dtype` is the precision of the tables and of every sum."""

    def __init__(self, dtype=torch.float64):
        self.dtype = dtype
        self.np = np.float64 if dtype == torch.float64 else np.float32

    def to_device(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def plan(self, rowptr, f, chunk=0, row_begin=0, row_end=None):
        return _Plan(rowptr, f, row_begin, row_end)

    def _sums(self, plan, colidx, val, gather, alpha):
        """(sum w y y^T, sum_{r>0} (1 + w) y, entries) of the plan's rows over the plan's entries."""
        b0, e0, f = plan.row_begin, plan.row_end, plan.f
        Y, ci, va = gather.numpy().astype(self.np), colidx.numpy(), val.numpy().astype(self.np)
        S, rhs = np.zeros((e0 - b0, f, f), self.np), np.zeros((e0 - b0, f), self.np)
        for u in range(b0, e0):
            s, e = plan.rowptr[u], plan.rowptr[u + 1]
            w = self.np(alpha) * np.abs(va[s:e])
            yu = Y[ci[s:e]]
            S[u - b0] = (yu * w[:, None]).T @ yu
            rhs[u - b0] = np.where(va[s:e] > 0, 1 + w, 0).astype(self.np) @ yu
        return S, rhs, np.diff(plan.rowptr[b0:e0 + 1])

    def gram(self, table, G):
        Y = table.numpy().astype(self.np)
        G.copy_(torch.from_numpy(Y.T @ Y))

    def update_implicit(self, plan, colidx, val, gather, G, update, lam, alpha, reg, solver, cg_iters):
        assert solver in ("cg", "lu", "cg_matfree")
        S, rhs, cnt = self._sums(plan, colidx, val, gather, alpha)
        f = plan.f
        diag = lam * cnt if reg == "weighted" else np.full(len(cnt), lam)
        A = G.numpy()[None] + S + diag[:, None, None].astype(self.np) * np.eye(f, dtype=self.np)
        A[cnt == 0] = np.eye(f)
        out = update.numpy()[plan.row_begin:plan.row_end]
        new = solve(A, rhs, out, "lu" if solver == "lu" else "cg", cg_iters)
        new[cnt == 0] = 0.0
        out[:] = new

    def hermitian_partial(self, plan, colidx, val, gather, lam, alpha, reg, packed, rhs):
        S, b, cnt = self._sums(plan, colidx, val, gather, alpha)
        if reg == "weighted":
            S += (lam * cnt)[:, None, None].astype(self.np) * np.eye(plan.f, dtype=self.np)
        iu = np.triu_indices(plan.f)
        packed.copy_(torch.from_numpy(np.ascontiguousarray(S[:, iu[0], iu[1]])))
        rhs.copy_(torch.from_numpy(b))

    def finish(self, packed, G, reg_add, tt):
        f = G.shape[-1]
        iu = np.triu_indices(f)
        A = np.zeros((packed.shape[0], f, f), self.np)
        A[:, iu[0], iu[1]] = packed.numpy()
        A[:, iu[1], iu[0]] = packed.numpy()
        A += G.numpy()[None]
        A += self.np(reg_add) * np.eye(f, dtype=self.np)
        tt.copy_(torch.from_numpy(A))

    def solve(self, tt, rhs, x, solver, cg_iters):
        assert solver in ("cg", "lu")
        new = solve(tt.numpy(), rhs.numpy(), x.numpy(), solver, cg_iters)
        x.copy_(torch.from_numpy(np.ascontiguousarray(new)))

    def loss(self, rowptr, colidx, val, XT, thetaT, lam, alpha, reg):
        return ref.sparse_loss(rowptr.numpy(), colidx.numpy(), val.numpy(), XT.numpy(), thetaT.numpy(), lam, alpha, reg)


def host_matrix(d, m, n):
    from cumf_als_amd import dist as cdist

    return cdist.HostMatrix(m, n, d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indptr"], d["csc_indices"],
                            d["csc_data"])


def worker(rank, world, port, configs, d, m, n, lam, alpha, iters, q, ops_kind="numpy"):
    """Entry point of one rank (spawned): one process group, then every configuration in `configs` -- dicts with scheme,
    solver, reg, theta_batch, f, theta0 -- through DistImplicitALS; the list of (thetaT, full XT, loss) goes back through
    `q`."""
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cumf_als_amd import dist_implicit as di

        if ops_kind == "hip":
            torch.cuda.set_device(0)
            ops = di.HipImplicitOps("cuda:0")
        else:
            ops = NumpyImplicitOps()
        out = []
        for c in configs:
            eng = di.DistImplicitALS(host_matrix(d, m, n), c["f"], lam, alpha, ops, solver=c["solver"], cg_iters=3,
                                     reg=c["reg"], scheme=c["scheme"], theta_batch=c["theta_batch"])
            eng.init_factors(c["theta0"])
            eng.iterate(iters)
            loss = eng.loss()
            out.append((eng.thetaT.cpu().numpy().copy(), eng.full_XT().cpu().numpy().copy(), loss))
            eng.close()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def run_ranks(world, configs, d, m, n, lam, alpha, iters, ops_kind="numpy", timeout=300):
    """Spawn `world` ranks of `worker`.  A child that exits non-zero fails the call at once (the others, which may wait for
    it in a collective, are killed), `timeout` seconds bound the whole run, nothing is retried.  Returns per rank the list
    of (thetaT, XT, loss) in the order of `configs`."""
    import queue
    import socket
    import time

    import torch.multiprocessing as mp

    from cumf_als_amd import dist_implicit  # noqa: F401  (a tree without the module fails here, before anything is spawned)

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(rk, world, port, configs, d, m, n, lam, alpha, iters, q, ops_kind))
             for rk in range(world)]
    for p in procs:
        p.start()
    outs = []
    deadline = time.monotonic() + timeout
    try:
        while len(outs) < world and time.monotonic() < deadline:
            try:
                outs.append(q.get(timeout=0.2))
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):
                    break
        if len(outs) == world:
            for p in procs:
                p.join(timeout=60)
    finally:
        codes = [p.exitcode for p in procs]
        for p in procs:
            if p.exitcode is None:
                p.kill()
                p.join(timeout=10)
    assert codes == [0] * world and len(outs) == world, (codes, len(outs))
    return [o for _, o in sorted(outs, key=lambda t: t[0])]


def run_ranks_once(cache, key, *args, **kwargs):
    """`run_ranks`, computed once per `key` and shared by the cases that read it; a failure is kept too, so that every case
    fails with it instead of spawning again."""
    if key not in cache:
        try:
            cache[key] = (run_ranks(*args, **kwargs), None)
        except BaseException as e:  # noqa: BLE001  (kept and re-raised for every case)
            cache[key] = (None, (e, e.__traceback__))
    out, err = cache[key]
    if err is not None:
        raise err[0].with_traceback(err[1])  # the first traceback, not one that grows with every case
    return out
