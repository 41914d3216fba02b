"""GPU parity: HIP path (through the C ABI of libALS.so) vs the CPU oracle.

Tolerances (stated per north_star "within a stated fp32 tolerance"):
  * Gram of a whole (unchunked) row, gram mode "exact": BIT-EXACT vs the oracle -- the fp32 MFMA is
    a k-ordered fmaf chain, the same chain a reference thread evaluates (als.h:39-143).
  * Gram, default mode (fp32 split exactly into 3 bf16 terms, 6 products on the bf16 matrix pipe,
    fp32 accumulate): max |G - G_fp64| <= 1e-6 * max|G| and no worse than 1.5x the fmaf chain's own distance
    from the fp64 Gram; on adversarial inputs (mixed signs, nine decades, cancelling right-hand sides,
    near-sub-normal products) bounded PER ENTRY by rho * 2^-24 * sum |theta_i theta_j| with rho <= 3 + 6 ceil(n_u / 32)
    per row and rms / q99.9 / max of rho within 1.1 x / 1.5 x / 2 x of the fmaf chain's
    (test_split_gram_adversarial_per_entry).
  * Gram of a chunked row: partial chains are summed -> rel 2e-6 of the row's scale.
  * LU solve on identical (A, b): the exact-order variant is bit-exact; the fast
    register-resident symmetric elimination agrees to 2e-5 relative.
  * CG solve: dot products are reduced in a different (deterministic) order ->
    ||x - x_oracle||_inf <= 2e-4 * max(1, ||x||_inf); RMSE parity 1e-4.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")


def _dataset(m, n, nnz, nnz_test, seed, **kw):
    from cumf_als_amd import datagen

    return datagen.synth_ratings(m, n, nnz, nnz_test, seed=seed, **kw)


def _factors(rows, f, seed):
    rng = np.random.RandomState(seed)
    return (0.2 * rng.random_sample((rows, f))).astype(np.float32)


@pytest.mark.parametrize("f", [10, 20, 30, 64, 80, 100, 120, 130, 160, 200])
def test_gram_whole_rows_bit_exact(oracle, alslib, f):
    _need_gpu()
    from cumf_als_amd import als

    als.set_gram_mode("exact")

    r = _dataset(96, 80, 1900, 300, seed=f)
    d = r.numpy()
    theta = _factors(r.n, f, 1)
    lam = 0.05
    tt_o, b_o = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    assert plan.n_multi_rows == 0
    tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), lam)
    torch.cuda.synchronize()
    als.set_gram_mode("auto")
    np.testing.assert_array_equal(tt.cpu().numpy(), tt_o)
    np.testing.assert_array_equal(rhs.cpu().numpy(), b_o)


@pytest.mark.parametrize("f", [20, 30, 48, 56, 64, 100, 110])
def test_split_gram_error_class(oracle, alslib, f):
    """Default Gram arithmetic (als_wave.hip): every fp32 value split exactly into three bf16
    terms, products hh + hm + mh + mm + hl + lh on v_mfma_f32_16x16x32_bf16, fp32 accumulation.
    Against the fp64 Gram it must sit in the same error class as the bit-exact fmaf chain."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(96, 400, 9000, 300, seed=f, row_alpha=1.2)
    d = r.numpy()
    theta = _factors(r.n, f, 1)
    lam = 0.05
    tt64, b64 = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam, dtype=np.float64)
    rg = r.to("cuda")
    th = torch.from_numpy(theta).cuda()
    plan = als.Plan(d["csr_indptr"], f)
    err = {}
    for mode in ("exact", "auto"):
        als.set_gram_mode(mode)
        tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, th, lam)
        torch.cuda.synchronize()
        err[mode] = (np.abs(tt.cpu().numpy() - tt64).max() / np.abs(tt64).max(),
                     np.abs(rhs.cpu().numpy() - b64).max() / np.abs(b64).max())
    als.set_gram_mode("auto")
    assert err["auto"][0] <= 1e-6 and err["auto"][1] <= 2e-6, err
    assert err["auto"][0] <= 1.5 * err["exact"][0] + 5e-8, err
    assert err["auto"][1] <= 1.5 * err["exact"][1] + 5e-8, err


def _adversarial_table(kind, n, f, rng):
    """Gather tables that a benign 0.2 * U[0, 1) draw never produces."""
    if kind == "mixed_sign":          # every off-diagonal Gram entry is a cancelling sum
        return rng.standard_normal((n, f)).astype(np.float32)
    if kind == "wide_range":          # nine decades inside every row, mixed signs
        mag = 10.0 ** rng.uniform(-6.0, 3.0, size=(n, f))
        return (mag * rng.choice([-1.0, 1.0], size=(n, f))).astype(np.float32)
    if kind == "cancel_pairs":        # rows 2k and 2k + 1 are theta and -theta + eps: the right-hand side cancels to r * eps
        base = rng.standard_normal((n // 2, f))
        t = np.empty((n, f))
        t[0::2] = base
        t[1::2] = -base + 1e-4 * rng.standard_normal((n // 2, f))
        return t.astype(np.float32)
    if kind == "tiny":                # products of 1e-30: the l terms are still normal numbers
        return (1e-15 * rng.standard_normal((n, f))).astype(np.float32)
    if kind == "near_subnormal":      # products of 1e-36: partial products l * h are sub-normal
        return (1e-18 * rng.standard_normal((n, f))).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["mixed_sign", "wide_range", "cancel_pairs", "tiny", "near_subnormal"])
@pytest.mark.parametrize("f", [30, 100, 110, 200])
def test_split_gram_adversarial_per_entry(oracle, alslib, kind, f):
    """VERDICT r02 item 1a.  The default Gram arithmetic (exact bf16x3 split, six products on the bf16 matrix
    pipe) on inputs chosen to hurt it -- mixed signs (cancelling sums), nine decades of magnitude inside a row,
    theta / -theta + eps pairs with equal ratings (the RHS cancels), non-integer ratings on a 0..100 scale,
    values whose partial products approach the fp32 sub-normal range -- bounded PER ENTRY against the fp64 Gram:

        |G_ij - G64_ij| <= rho * 2^-24 * sum_k |theta_ki theta_kj|  (+ n_u * 2^-126: one minimum normal per rating)

    with, per row, rho <= 3 + 6 ceil(n_u / 32): six fp32 accumulator roundings per 32-rating stage (each at most one
    unit of the running |sum| <= sum |.|), two units for the dropped ml + lm + ll terms, one for the matrix pipe's
    internal 32-term sum -- a WORST-CASE bound of the same form as, and five times tighter than, the fmaf chain's own
    n_u * 2^-24 (Higham); and, entry by entry against the bit-exact fmaf chain (gram mode "exact", same inputs):
        rms(rho_split) <= 1.1 rms(rho_chain),  q99.9 <= 1.5 x,  max <= 2 x  (or <= 3 units when the chain is exact)
    Measured (profiles/r03/calib_adversarial.txt): rms ratio 0.85 .. 1.04, q99.9 ratio 0.94 .. 1.20, max ratio
    0.95 .. 1.64; one product alone (n_u = 1) 1.4 .. 2.6 units.  The maximum over 5 * 10^5 entries is an extreme-value
    statistic (the chain's own maximum moves by 1.5 x between seeds), hence 2 x there and 1.5 x on the quantile.
    Near the sub-normal range the floor is n_u * 2^-126.  Rows of 1, 31, 32, 33 ... 1500 ratings."""
    _need_gpu()
    from cumf_als_amd import als

    rng = np.random.RandomState(1000 + f)
    n = 1600
    lens = np.array([1, 2, 31, 32, 33, 63, 64, 65, 100, 206, 400, 777, 1500] + list(rng.randint(1, 300, size=35)))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    table = _adversarial_table(kind, n, f, rng)
    cols, vals = [], []
    for k in lens:
        if kind == "cancel_pairs":   # both members of a pair, with the same rating
            pairs = rng.choice(n // 2, size=(k + 1) // 2, replace=False)
            c = np.sort(np.concatenate([2 * pairs, 2 * pairs + 1])[:k])
            rv = 100.0 * rng.random_sample(n // 2)
            v = rv[c // 2]
        else:
            c = np.sort(rng.choice(n, size=k, replace=False))
            v = 100.0 * rng.random_sample(k)       # non-integer, 0..100
        cols.append(c)
        vals.append(v)
    indices = np.concatenate(cols).astype(np.int32)
    data = np.concatenate(vals).astype(np.float32)
    lam = 0.0   # the regulariser would hide the small entries of the diagonal
    tt64, b64 = oracle.gram_rhs(indptr, indices, data, table, f, lam, dtype=np.float64)
    # sum_k |theta_ki| |theta_kj| and sum_k |r_k| |theta_ki|: the same oracle on the absolute values
    ab64, abb64 = oracle.gram_rhs(indptr, indices, np.abs(data), np.abs(table), f, lam, dtype=np.float64)
    u = 2.0 ** -24
    floor = lens.astype(np.float64) * 2.0 ** -126
    dev = lambda a: torch.from_numpy(a).cuda()
    plan = als.Plan(indptr, f)
    assert plan.n_multi_rows == 0
    rho = {}
    try:
        for mode in ("exact", "auto"):
            als.set_gram_mode(mode)
            tt, rhs = als.get_hermitian(plan, dev(indices), dev(data), dev(table), lam)
            torch.cuda.synchronize()
            eg = np.abs(tt.cpu().numpy().astype(np.float64) - tt64) / (u * ab64 + floor[:, None, None])
            eb = np.abs(rhs.cpu().numpy().astype(np.float64) - b64) / (u * abb64 + floor[:, None])
            rho[mode] = (eg.reshape(len(lens), -1), eb)
    finally:
        als.set_gram_mode("auto")
    stat = lambda v: (float(np.sqrt((v * v).mean())), float(np.quantile(v, 0.999)), float(v.max()))
    msg = {m: {"gram (rms, q99.9, max)": stat(v[0]), "rhs": stat(v[1])} for m, v in rho.items()}
    print(f"rho[{kind}, f={f}]:", msg)
    bound = 3.0 + 6.0 * np.ceil(lens / 32.0)
    for k in (0, 1):   # Gram entries, right-hand sides
        a, e = rho["auto"][k], rho["exact"][k]
        assert (a.max(1) <= bound).all(), (msg, (a.max(1) / bound).max())
        (a_rms, a_q, a_max), (e_rms, e_q, e_max) = stat(a), stat(e)
        assert a_rms <= max(1.1 * e_rms, 0.5), msg
        assert a_q <= max(1.5 * e_q, 3.0), msg
        assert a_max <= max(2.0 * e_max, 3.0), msg


@pytest.mark.parametrize("f", [20, 64, 100, 128, 200])
def test_fast_gram_error_class(oracle, alslib, f):
    """Opt-in gram mode "fast" (pre-split (h, l) f16 pairs, products hh + hl + lh, 22 significand bits):
    the LU solution of a half-iteration against the fp64 solution of the fp64 normal equations must stay
    in the fp32 class -- within 1e-5 relative and within 4x the distance of the default (24-bit) arithmetic
    -- and the range flags must stay clear."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(96, 400, 9000, 300, seed=f, row_alpha=1.2)
    d = r.numpy()
    theta = _factors(r.n, f, 1)
    lam = 0.05
    tt64, b64 = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam, dtype=np.float64)
    x64 = np.linalg.solve(tt64, b64[..., None])[..., 0]
    rg = r.to("cuda")
    th = torch.from_numpy(theta).cuda()
    plan = als.Plan(d["csr_indptr"], f)
    err = {}
    try:
        for mode in ("auto", "fast"):
            als.set_gram_mode(mode)
            x = torch.zeros((r.m, f), device="cuda")
            als.update_fused(plan, rg.csr_indices, rg.csr_data, th, x, lam, "lu", 6)
            torch.cuda.synchronize()
            err[mode] = np.abs(x.cpu().numpy() - x64).max() / np.abs(x64).max()
        assert als.gram_fast_status() == 0
    finally:
        als.set_gram_mode("auto")
    assert err["fast"] <= 1e-5, err
    assert err["fast"] <= 4 * err["auto"] + 1e-6, err


def test_fast_gram_range_flags(alslib):
    """Gram mode "fast" reports, on the device, a factor (bit 0) or a rating (bit 1) that leaves the f16
    range of the pre-split words (|value| >= 15.99) instead of returning silently wrong factors."""
    _need_gpu()
    from cumf_als_amd import als

    f = 32
    r = _dataset(64, 80, 2000, 100, seed=3)
    d = r.numpy()
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    try:
        als.set_gram_mode("fast")
        als.gram_fast_status()
        theta = _factors(r.n, f, 2)
        x = torch.zeros((r.m, f), device="cuda")
        als.update_fused(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), x, 0.05, "lu", 6)
        assert als.gram_fast_status() == 0
        big = theta.copy()
        big[5, 3] = 40.0
        als.update_fused(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(big).cuda(), x, 0.05, "lu", 6)
        assert als.gram_fast_status() & 1
        vals = rg.csr_data.clone()
        vals[7] = 100.0
        als.update_fused(plan, rg.csr_indices, vals, torch.from_numpy(theta).cuda(), x, 0.05, "lu", 6)
        assert als.gram_fast_status() & 2
        assert als.gram_fast_status() == 0  # reading clears
        # the engine raises instead of returning non-finite factors
        import dataclasses

        bad = dataclasses.replace(rg, csr_data=vals)
        eng = als.ALSEngine(bad, f, 0.05, solver="lu")
        eng.init_factors(theta)
        with pytest.raises(RuntimeError, match="f16 range"):
            eng.iterate(1)
        # doALS itself: returns NaN + cumf_last_error() == CUMF_ERR_FAST_RANGE instead of exiting from library code
        # (ADVICE r02); the Python mirror raises
        db = bad.numpy()
        with pytest.raises(RuntimeError, match="f16 range"):
            als.do_als(db["csr_indptr"], db["csr_indices"], db["csr_data"], db["csc_indices"], db["csc_indptr"],
                       db["csc_data"], db["coo_row"], db["test_row"], db["test_col"], db["test_data"], r.m, r.n, f,
                       r.nnz, r.nnz_test, 0.05, 2, 1, 1, 0, solver="lu")
        assert alslib.cumf_last_error() == 0   # reading cleared it
    finally:
        als.set_gram_mode("auto")


def test_fast_gram_tolerates_nan_rows_of_empty_columns(alslib):
    """rows / columns without ratings get NaN factors by design (0/0 in CG, a zero pivot in LU:
    cg.cu:128; test_empty_row_gives_nan_like_reference).  Their table rows are never gathered, so gram mode
    "fast" must run on such a dataset -- sparse id spaces like ML-10M's n = 65 133 -- without raising."""
    _need_gpu()
    from cumf_als_amd import als, datagen

    f, m, n = 32, 40, 30
    rng = np.random.RandomState(5)
    rows = rng.randint(0, m, 600)
    cols = rng.randint(0, n - 3, 600)          # columns n-3 .. n-1 have no rating at all
    keep = np.unique(rows * n + cols)
    rows, cols = keep // n, keep % n
    r = datagen.from_coo(m, n, rows, cols, rng.randint(1, 6, len(rows)).astype(np.float32), [0], [0], [1.0]).to("cuda")
    try:
        als.set_gram_mode("fast")
        als.gram_fast_status()
        eng = als.ALSEngine(r, f, 0.05, solver="lu")
        eng.init_factors()
        eng.iterate(3)          # raises on a range flag
        torch.cuda.synchronize()
        th = eng.thetaT.cpu().numpy()
        assert np.isnan(th[n - 3:]).all() and np.isfinite(th[: n - 3]).all() and np.isfinite(eng.XT.cpu().numpy()).all()
        assert als.gram_fast_status() == 0
    finally:
        als.set_gram_mode("auto")


def test_packed_gram_equals_pack_of_full(alslib):
    """cumf_get_hermitian_packed writes the packed upper triangles straight from the accumulators: bit-identical
    to cumf_get_hermitian + cumf_pack_upper, whole rows and chunked rows, wave and workgroup kernels."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(60, 300, 5000, 300, seed=9, row_alpha=1.3)
    d = r.numpy()
    rg = r.to("cuda")
    try:
        for mode in ("auto", "exact"):
            als.set_gram_mode(mode)
            for f, chunk in ((10, 0), (20, 32), (100, 0), (100, 64), (128, 0), (200, 96)):
                theta = torch.from_numpy(_factors(r.n, f, 2) - 0.1).cuda()
                plan = als.Plan(d["csr_indptr"], f, chunk=chunk)
                tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, theta, 0.05)
                pk, rhs2 = als.get_hermitian_packed(plan, rg.csr_indices, rg.csr_data, theta, 0.05)
                torch.cuda.synchronize()
                assert torch.equal(pk, als.pack_upper(tt)), (mode, f, chunk)
                assert torch.equal(rhs, rhs2), (mode, f, chunk)
    finally:
        als.set_gram_mode("auto")


def test_dispatched_kernel_name_and_committed_traffic(alslib):
    """bench.py's roofline.kernel is the symbol that was dispatched (cumf_last_kernel_name), and the committed
    PMC traffic (profiles/traffic.json) is keyed by that name: the headline kernel must be in it."""
    _need_gpu()
    import json
    import os

    from cumf_als_amd import als

    r = _dataset(64, 80, 2000, 100, seed=3).to("cuda")
    d = r.numpy()
    x = torch.zeros((r.m, 100), device="cuda")
    theta = torch.from_numpy(_factors(r.n, 100, 1)).cuda()
    als.update_fused(als.Plan(d["csr_indptr"], 100), r.csr_indices, r.csr_data, theta, x, 0.05, "lu", 6)
    name = als.last_kernel_name()
    assert name.startswith("cumf::als_wave_kernel<7, 1, 100"), name
    als.update_fused(als.Plan(d["csr_indptr"], 100), r.csr_indices, r.csr_data, theta, x, 0.05, "cg", 6)
    assert als.last_kernel_name().startswith("cumf::als_wave_kernel<7, 0, 100"), als.last_kernel_name()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = json.load(open(os.path.join(root, "profiles", "traffic.json")))
    # (this small plan has no chunked row, so `name` is the WHOLE instance: the Theta-side kernel of the headline
    # profile; its X side dispatches the sibling instance)
    have = [n.replace(" ", "") for e in table["kernels"]
            for n in (e["kernel"], e.get("x_side", {}).get("kernel", ""), e.get("theta_side", {}).get("kernel", ""))]
    assert name.replace(" ", "") in have, (name, have)
    # the ablation switches are not part of the product library
    assert not hasattr(alslib, "cumf_set_debug_switches")
    with pytest.raises(RuntimeError):
        als.set_debug_switches(1)


def test_bench_plain_line_and_full_legs(alslib, tmp_path):
    """bench.py without --full prints the headline line alone -- the same keys, dtype and dumped factors as a --full run of
    the same steps -- and --full adds the roofline, RMSE, gram-mode, CPU-baseline and parity legs behind them."""
    _need_gpu()
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines, dumps = {}, {}
    for tag, extra in (("plain", []), ("full", ["--full"])):
        out_dir = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--scale", "0.05", "--dump-outputs", out_dir] + extra
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, out.stderr[-3000:]
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(got) == 1, out.stdout[-2000:]
        lines[tag] = json.loads(got[0])
        dumps[tag] = {k: np.load(os.path.join(out_dir, k + ".npy")) for k in ("x", "theta")}
    plain, full = lines["plain"], lines["full"]
    legs = {"roofline", "rmse", "gram_fast_mode", "gram_exact_mode", "cpu_baseline", "parity_at_scale"}
    assert legs <= set(full), sorted(full)
    assert set(plain) == set(full) - legs, sorted(plain)
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "data"):
        assert plain[k] == full[k], (k, plain[k], full[k])
    assert plain["config"]["workload"] == full["config"]["workload"]
    assert plain["dtype"] == "f32 (bf16x3-split products on the bf16 matrix pipe, fp32 accumulate)", plain["dtype"]
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    for k in ("x", "theta"):  # the timed steps and what they leave behind do not depend on --full
        assert np.array_equal(dumps["plain"][k], dumps["full"][k], equal_nan=True), k


def test_whole_row_kernel_is_bit_identical_to_the_combined_one(alslib):
    """The LU wave kernel has two instances: WHOLE (the plan has no chunked row: no partial-tile exit, 0 spills) and
    the combined one (a plan whose chunked rows hold a quarter or more of its ratings: one launch, the whole rows fill the
    tail of the chunk items).  The same rows must come out bit for bit from both: a plan of short rows alone (WHOLE)
    against the same rows in a plan that also holds one row long enough to be chunked and to dominate the plan."""
    _need_gpu()
    from cumf_als_amd import als

    f, lam = 100, 0.05
    rng = np.random.RandomState(11)
    n = 9000
    short = list(rng.randint(1, 400, size=40))
    theta = torch.from_numpy(_factors(n, f, 3) - 0.08).cuda()
    out = {}
    for tag, lens in (("whole", short), ("combined", short + [8000])):
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        r2 = np.random.RandomState(5)   # same draws for the common rows (indices and ratings row by row)
        cols, vals = [], []
        for k in lens:
            cols.append(np.sort(r2.choice(n, size=k, replace=False)))
            vals.append(r2.randint(1, 6, size=k))
        indices = np.concatenate(cols).astype(np.int32)
        data = np.concatenate(vals).astype(np.float32)
        plan = als.Plan(indptr, f, chunk=512)
        assert (plan.n_multi_rows == 0) == (tag == "whole")
        x = torch.zeros((len(lens), f), device="cuda")
        als.update_fused(plan, torch.from_numpy(indices).cuda(), torch.from_numpy(data).cuda(), theta, x, lam, "lu", 6)
        torch.cuda.synchronize()
        name = als.last_kernel_name()
        assert name.endswith("true>" if tag == "whole" else "false>"), name
        out[tag] = x[: len(short)].cpu().numpy()
    # (the column draws of the common rows are identical only if the long row is drawn last: it is)
    np.testing.assert_array_equal(out["whole"], out["combined"])


def test_long_row_many_slots(oracle, alslib):
    """A row of 210 000 ratings (Netflix X-side scale: rows of 10^5 ratings cut into ~100 chunks, the
    reduce kernel summing ~100 partial tile sets in slot order) against the fp64 oracle."""
    _need_gpu()
    from cumf_als_amd import als

    f, lam = 100, 0.048
    lens = [210_000, 5_000, 33]
    n = lens[0]
    rng = np.random.RandomState(3)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in lens]).astype(np.int32)
    data = rng.randint(1, 6, size=indptr[-1]).astype(np.float32)
    theta = _factors(n, f, 4)
    tt64, b64 = oracle.gram_rhs(indptr, indices, data, theta, f, lam, dtype=np.float64)
    x64 = np.linalg.solve(tt64.astype(np.float64), b64[..., None])[..., 0]
    dev = lambda a: torch.from_numpy(a).cuda()
    plan = als.Plan(indptr, f)
    assert plan.n_slots >= 49 and plan.n_multi_rows == 2, (plan.n_slots, plan.n_multi_rows)
    for mode in ("exact", "auto"):
        als.set_gram_mode(mode)
        tt, rhs = als.get_hermitian(plan, dev(indices), dev(data), dev(theta), lam)
        x = torch.zeros((3, f), device="cuda")
        als.update_fused(plan, dev(indices), dev(data), dev(theta), x, lam, "lu", 6)
        torch.cuda.synchronize()
        assert np.abs(tt.cpu().numpy() - tt64).max() <= 2e-6 * np.abs(tt64).max(), mode
        assert np.abs(rhs.cpu().numpy() - b64).max() <= 2e-6 * np.abs(b64).max(), mode
        assert np.abs(x.cpu().numpy() - x64).max() <= 1e-4 * np.abs(x64).max(), mode
    als.set_gram_mode("auto")


def test_gather_table_guard(alslib):
    """VERDICT r01 / ADVICE r01: the 32-bit gather offsets of the workgroup kernels must fail loudly
    at 4 GiB; the wave kernels (LU, f <= 111) address with 64 bits."""
    from cumf_als_amd import als

    rows = (1 << 32) // 400 + 1  # 10.7 M rows at f = 100
    als.set_gram_mode("auto")
    assert alslib.cumf_check_gather_table(rows, 100, als.SOLVER_LU, 0) == 0
    assert alslib.cumf_check_gather_table(rows, 100, als.SOLVER_CG, 0) == 0   # wave kernels: 64-bit lane addresses
    assert alslib.cumf_check_gather_table(rows, 200, als.SOLVER_LU, 0) == 0   # two-waves-per-item Gram: 64-bit
    assert alslib.cumf_check_gather_table((1 << 32) // 40 + 1, 10, als.SOLVER_LU, 0) != 0  # f = 10: workgroup kernels
    als.set_gram_mode("exact")
    assert alslib.cumf_check_gather_table(rows, 100, als.SOLVER_LU, 0) != 0
    assert alslib.cumf_check_gather_table(rows - 2, 100, als.SOLVER_LU, 0) == 0
    als.set_gram_mode("auto")


@pytest.mark.parametrize("gram_mode", ["exact", "auto"], indirect=True)
@pytest.mark.parametrize("f,chunk", [(100, 32), (100, 64), (20, 32), (64, 96), (128, 64), (160, 32)])
def test_gram_chunked_rows(oracle, alslib, gram_mode, f, chunk):
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(40, 300, 4000, 300, seed=3, row_alpha=1.3)
    d = r.numpy()
    theta = _factors(r.n, f, 2)
    lam = 0.048
    tt_o, b_o = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam, dtype=np.float64)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f, chunk=chunk)
    assert plan.n_multi_rows > 0 and plan.n_slots > plan.n_multi_rows
    tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), lam)
    torch.cuda.synchronize()
    scale = np.abs(tt_o).max()
    assert np.abs(tt.cpu().numpy() - tt_o).max() <= 2e-6 * scale
    assert np.abs(rhs.cpu().numpy() - b_o).max() <= 2e-6 * np.abs(b_o).max()


@pytest.mark.parametrize("f", [10, 40, 100, 128, 200])
def test_lu_solve(oracle, alslib, f, monkeypatch):
    """Batched unpivoted LU.  CUMF_ALS_LU_EXACT=1 (LDS elimination in the oracle's operation
    order): bit-exact.  Default (register-resident symmetric
    elimination, l = u_ki * (1/u_kk)): same solution to 2e-5 relative."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(64, 90, 2500, 300, seed=5)
    d = r.numpy()
    theta = _factors(r.n, f, 3)
    A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, 0.05)
    x_o = oracle.lu(A, b, f)
    Ag, bg = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    monkeypatch.setenv("CUMF_ALS_LU_EXACT", "1")
    x = als.lu_solve(Ag, bg)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(x.cpu().numpy(), x_o)
    monkeypatch.delenv("CUMF_ALS_LU_EXACT")
    x = als.lu_solve(Ag, bg)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Ag.cpu().numpy(), A)  # A is not modified
    err = np.abs(x.cpu().numpy() - x_o).max()
    assert err <= 2e-5 * np.abs(x_o).max(), err


@pytest.mark.parametrize("f", [10, 40, 100, 128, 200])
def test_cg_solve(oracle, alslib, f):
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(64, 90, 2500, 300, seed=6)
    d = r.numpy()
    theta = _factors(r.n, f, 4)
    A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, 0.05)
    x0 = _factors(r.m, f, 9) * 0.1
    x_o = oracle.cg(A, x0, b, f, 6)
    x = torch.from_numpy(x0.copy()).cuda()
    als.cg_solve(torch.from_numpy(A).cuda(), x, torch.from_numpy(b).cuda(), 6)
    torch.cuda.synchronize()
    err = np.abs(x.cpu().numpy() - x_o).max()
    assert err <= 2e-4 * max(1.0, np.abs(x_o).max()), err
    # the tolerance stated on the residual.  After the same <= 6 iterations the HIP
    # iterate must be as good a solution as the oracle's: ||A x - b|| within 1e-4 ||b|| of the
    # oracle's residual per system (the dot products differ only in summation order).
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    res_h = np.linalg.norm(np.einsum("bij,bj->bi", A64, x.cpu().numpy().astype(np.float64)) - b64, axis=1)
    res_o = np.linalg.norm(np.einsum("bij,bj->bi", A64, x_o.astype(np.float64)) - b64, axis=1)
    assert (np.abs(res_h - res_o) <= 1e-4 * np.linalg.norm(b64, axis=1)).all(), np.abs(res_h - res_o).max()


@pytest.mark.parametrize("f", [100, 20])
def test_reference_cxx_entry_points(oracle, alslib, f):
    """The C++-linkage symbols a caller compiled against the reference's cg.h binds, called as that caller would
    (device pointers, synchronous): updateXWithCGHost (cg.h:30), updateXWithCGHost_tt_fp16 (cg.h:32) and the fused
    Gram + CG host alsUpdateFeature100Host (cg.h:34-36) with a batch offset."""
    _need_gpu()
    import ctypes as C

    from cumf_als_amd import als

    r = _dataset(64, 90, 2500, 300, seed=16)
    d = r.numpy()
    theta = _factors(r.n, f, 4)
    lam = 0.05
    A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam)
    x0 = _factors(r.m, f, 9) * 0.1
    x_o = oracle.cg(A, x0, b, f, 6)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    cg = getattr(alslib, "_Z17updateXWithCGHostPfS_S_iif")
    cg.restype = None
    cg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    Ad, bd = torch.from_numpy(A).cuda(), torch.from_numpy(b).cuda()
    x = torch.from_numpy(x0.copy()).cuda()
    cg(ptr(Ad), ptr(x), ptr(bd), r.m, f, 6.0)   # synchronous: no torch.cuda.synchronize() before the read
    assert np.abs(x.cpu().numpy() - x_o).max() <= 2e-4 * max(1.0, np.abs(x_o).max())

    cg16 = getattr(alslib, "_Z25updateXWithCGHost_tt_fp16PfS_S_iif")
    cg16.restype = None
    cg16.argtypes = cg.argtypes
    A16 = A.astype(np.float16)
    x16_o = oracle.cg(A16.astype(np.float32), x0, b, f, 6)
    x = torch.from_numpy(x0.copy()).cuda()
    cg16(ptr(torch.from_numpy(A16).cuda()), ptr(x), ptr(bd), r.m, f, 6.0)
    assert np.abs(x.cpu().numpy() - x16_o).max() <= 2e-4 * max(1.0, np.abs(x16_o).max())

    fused = getattr(alslib, "_Z23alsUpdateFeature100HostiPKiS0_fiiPKfPfS3_i")
    fused.restype = None
    fused.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_int]
    off = 5
    rg = r.to("cuda")
    rowptr = torch.from_numpy(d["csr_indptr"].astype(np.int32)).cuda()
    # batch-local XT / ythetaT: system k is row off + k
    x = torch.from_numpy(x0[off:].copy()).cuda()
    y = torch.from_numpy(b[off:].copy()).cuda()
    fused(off, ptr(rowptr), ptr(rg.csr_indices), lam, r.m, f, ptr(torch.from_numpy(theta).cuda()), ptr(x), ptr(y), 6)
    err = np.abs(x.cpu().numpy() - x_o[off:]).max()
    assert err <= 2e-4 * max(1.0, np.abs(x_o).max()), err
    assert als.last_kernel_name() != ""


@pytest.mark.parametrize("gram_mode", ["exact", "auto", "fast"], indirect=True)
@pytest.mark.parametrize("solver,f", [("cg", 10), ("cg", 100), ("cg", 128), ("lu", 10), ("lu", 100), ("lu", 128),
                                      ("lu", 200), ("lu", 98), ("lu", 110), ("lu", 96), ("lu", 206), ("cg", 98),
                                      # NB = 4 (f = 48 .. 63), the one instance of the one-wave kernels -- and of
                                      # the four-product diagonal tiles' doubled plane -- no matrix covered; NB = 5 with a strip
                                      ("lu", 48), ("lu", 56), ("cg", 48), ("cg", 56), ("lu", 64), ("lu", 68)])
def test_fused_half_iteration(oracle, alslib, gram_mode, solver, f):
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(200, 150, 9000, 600, seed=7, row_alpha=1.1)
    d = r.numpy()
    theta = _factors(r.n, f, 5)
    x0 = _factors(r.m, f, 6) * 0.05
    lam = 0.05
    x_o = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam,
                                solver=solver)
    rg = r.to("cuda")
    if solver == "cg":
        A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam)
        A64, b64 = A.astype(np.float64), b.astype(np.float64)
        res_o = np.linalg.norm(np.einsum("bij,bj->bi", A64, x_o.astype(np.float64)) - b64, axis=1)
    for chunk in (0, 64):
        plan = als.Plan(d["csr_indptr"], f, chunk=chunk)
        x = torch.from_numpy(x0.copy()).cuda()
        als.update_fused(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), x, lam, solver, 6)
        torch.cuda.synchronize()
        xh = x.cpu().numpy()
        err = np.abs(xh - x_o).max()
        if solver == "lu":
            # the elimination is the same factorisation in another rounding order (2e-5 on
            # identical (A, b)); on top sits the Gram arithmetic of the mode: 1e-4 RELATIVE, no absolute floor
            assert err <= 1e-4 * np.abs(x_o).max(), (chunk, err, np.abs(x_o).max())
        else:
            # CG(6): the tolerance lives on the residual.  After the same <= 6 iterations the HIP
            # iterate is as good a solution as the oracle's: ||A x - b|| within 1e-4 ||b|| of the oracle's, per
            # system -- no absolute floor (round 5) except where the stopping rule itself makes two iterates
            # interchangeable: the loop leaves as soon as ||r||^2 < CG_ERROR = 1e-4 (cg.cu:31,195), so when BOTH final
            # residuals are below sqrt(CG_ERROR) = 1e-2 one of the two may simply have stopped a step earlier
            res_h = np.linalg.norm(np.einsum("bij,bj->bi", A64, xh.astype(np.float64)) - b64, axis=1)
            close = np.abs(res_h - res_o) <= 1e-4 * np.linalg.norm(b64, axis=1) + 1e-6
            both_stopped = np.maximum(res_h, res_o) <= 1.05e-2
            assert (close | both_stopped).all(), (chunk, np.abs(res_h - res_o)[~(close | both_stopped)].max())
            # element-wise: 5e-4 of the factors' scale -- or, where the truncated recurrence is itself that sensitive (f = 48
            # with rows of fewer ratings than features, round 6: the fp32 oracle leaves its own fp64 evaluation by 1e-3
            # there), no further from the fp64 iterate than twice the fp32 oracle is (the yardstick of the full-size tests)
            if err > 5e-4 * max(1.0, np.abs(x_o).max()):
                x64 = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam,
                                            solver=solver, dtype=np.float64)
                e_o, e_h = np.abs(x_o - x64).max(), np.abs(xh - x64).max()
                assert e_h <= 2.0 * e_o + 1e-5, (chunk, err, e_h, e_o)


@pytest.mark.parametrize("f", [32, 48, 64, 100, 110])
def test_short_rows_gram_free_cg(oracle, alslib, f):
    """Round 6 (als_short.hip): whole rows of at most 32 ratings run the reference's CG (cg.cu:36-231) on A = T^T T + lambda n I
    without forming A -- u = T p by a transposing wave reduction, y = T^T u by broadcasts.  Rows of every length around
    the kernel's internal sizes (8 / 16 / 32 ratings in flight), an empty row, and rows just above the limit (Gram route) in ONE
    plan: NaN pattern of the reference (cg.cu:128), per row no further from the fp64 iterate than twice the fp32 oracle is
    (the full-size tests' yardstick; measured: closer than the Gram route), and the fused train SSE -- S - x.b - x.r -
    lambda n |x|^2 from the kernel's own vectors -- equal to the fp64 sum over the ratings on the returned factors."""
    _need_gpu()
    from cumf_als_amd import als, datagen

    lens = [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 20, 24, 25, 31, 32, 33, 40, 64, 65, 100] * 3
    n_cols = 160
    rng = np.random.RandomState(11)
    rows, cols, vals = [], [], []
    for u, ln in enumerate(lens):
        c = np.sort(rng.choice(n_cols, ln, replace=False))
        rows += [u] * ln
        cols += c.tolist()
        vals += rng.randint(1, 6, ln).astype(np.float32).tolist()
    r = datagen.from_coo(len(lens), n_cols, rows, cols, vals, [0], [0], [1.0])
    d = r.numpy()
    theta = _factors(n_cols, f, 5)
    x0 = _factors(len(lens), f, 6) * 0.05
    lam = 0.05
    x32 = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam, solver="cg")
    x64 = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam, solver="cg",
                                dtype=np.float64)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    x = torch.from_numpy(x0.copy()).cuda()
    bins = als.update_fused_sse(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), x, lam, "cg", 6)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    assert np.array_equal(np.isnan(xh), np.isnan(x64)) and np.isnan(xh[0]).all()
    fin = ~np.isnan(x64).any(1)
    e_o = np.abs(x32[fin] - x64[fin]).max(1)
    e_h = np.abs(xh[fin] - x64[fin]).max(1)
    scale = np.abs(x64[fin]).max()
    # two fp32 evaluations of six CG steps differ row by row (rows of fewer ratings than features: the recurrence divides
    # rounding noise by rounding noise once the n + 1 steps that solve the row are over), so the comparison is between the
    # DISTRIBUTIONS over the rows, as in tests/test_gpu_fullsize.py: median, 90th percentile and maximum of the distance from
    # the fp64 iterate no larger than the fp32 oracle's own, + 1e-5 of the factors' scale
    stats = lambda v: (float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max()))
    short = np.asarray(lens)[fin] <= 32
    print(f"short rows f={f}: |x - x64| (median, q90, max) hip {stats(e_h[short])} oracle32 {stats(e_o[short])}; "
          f"longer rows hip {stats(e_h[~short])} oracle32 {stats(e_o[~short])}")
    for sh, so in zip(stats(e_h[short]), stats(e_o[short])):
        assert sh <= 1.05 * so + 1e-5 * scale, (f, stats(e_h[short]), stats(e_o[short]))
    # train SSE of the finite rows on the returned factors, fp64
    ptr, idx, val = d["csr_indptr"], d["csr_indices"], d["csr_data"].astype(np.float64)
    sse = 0.0
    for u in np.nonzero(fin)[0]:
        pred = theta[idx[ptr[u]:ptr[u + 1]]].astype(np.float64) @ xh[u].astype(np.float64)
        sse += float(((val[ptr[u]:ptr[u + 1]] - pred) ** 2).sum())
    got = float(bins.sum().item())
    assert abs(got - sse) <= 2e-5 * sse, (got, sse)


def test_empty_row_gives_nan_like_reference(oracle, alslib):
    """cg.cu:128: alpha = 0/0 on an all-zero system -> NaN factors (same in the oracle)."""
    _need_gpu()
    from cumf_als_amd import als, datagen

    rows = [0, 0, 2, 2, 2]
    cols = [0, 1, 0, 1, 2]
    r = datagen.from_coo(3, 3, rows, cols, [1, 2, 3, 4, 5], [0], [0], [1.0])
    d = r.numpy()
    f = 10
    theta = _factors(3, f, 1)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    for solver in ("cg", "lu"):
        x = torch.zeros((3, f), device="cuda")
        als.update_fused(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), x, 0.05, solver, 6)
        xo = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta,
                                   np.zeros((3, f), np.float32), f, 0.05, solver=solver)
        xh = x.cpu().numpy()
        assert np.isnan(xh[1]).all() and np.isnan(xo[1]).all()
        assert np.isfinite(xh[[0, 2]]).all()


@pytest.mark.parametrize("f,solver", [(200, "cg"), (200, "lu"), (130, "cg"), (160, "lu")])
def test_doals_large_f(oracle, alslib, f, solver):
    """BASELINE config 3 (f = 200, CG(6) vs LU; test_als.sh:28) end to end through doALS: CG at
    f > 128 takes the unfused path (Gram batch at NB = 13 in HBM + cg_global_kernel), LU the fused
    workgroup kernels.  Two iterations against the oracle."""
    _need_gpu()
    from cumf_als_amd import als

    m, n, nnz, nnz_test, lam = 150, 120, 9000, 600, 0.05
    r = _dataset(m, n, nnz, nnz_test, seed=2)
    d = r.numpy()
    th0, x0 = oracle.init_factors(m, n, f)
    th_o, x_o = th0.copy(), x0.copy()
    rm_o, log_o = oracle.do_als(d, th_o, x_o, m, n, f, lam, 2, solver=solver)
    th64, x64 = th0.copy(), x0.copy()
    _, log_64 = oracle.do_als(d, th64, x64, m, n, f, lam, 2, solver=solver, dtype=np.float64)
    th, x, rm, log = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"],
                                d["csc_data"], d["coo_row"], d["test_row"], d["test_col"], d["test_data"], m, n, f,
                                r.nnz, r.nnz_test, lam, 2, 1, 1, 0, thetat_init=th0, xt_init=x0, solver=solver,
                                return_log=True)
    if solver == "lu":
        assert np.abs(th - th_o).max() <= 1e-4 * np.abs(th_o).max()
        assert np.abs(x - x_o).max() <= 1e-4 * np.abs(x_o).max()
        assert np.abs(log - log_o).max() <= 2e-5
    else:
        # 75 ratings per row at f = 200: under-determined rows, threshold-stopped CG -> the bound is
        # the oracle's own fp32-vs-fp64 spread (same rule as test_sse_and_doals_rmse)
        floor = np.abs(log_64 - log_o).max()
        assert np.abs(log - log_o).max() <= max(1e-4, floor), (np.abs(log - log_o).max(), floor)
        assert abs(rm - rm_o) <= max(1e-4, floor)


@pytest.mark.parametrize("gram_mode", ["exact", "auto", "fast"], indirect=True)
@pytest.mark.parametrize("shape", [(400, 300, 40000, 3000, 20), (300, 200, 6000, 700, 20)])
def test_sse_and_doals_rmse(oracle, alslib, gram_mode, shape):
    """Full doALS (5 iterations) vs the oracle.  LU: factors bit-identical.  CG: RMSE
    parity 1e-4 on the well-posed set; on the under-determined one (20 ratings per row at
    f = 20) the truncated CG is chaotic at fp32 level, so the bound is the oracle's own
    fp32-vs-fp64 spread."""
    _need_gpu()
    from cumf_als_amd import als

    m, n, nnz, nnz_test, f = shape
    lam = 0.05
    r = _dataset(m, n, nnz, nnz_test, seed=1)
    d = r.numpy()
    th0, x0 = oracle.init_factors(m, n, f)

    def run(**kw):
        return als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"],
                          d["csc_data"], d["coo_row"], d["test_row"], d["test_col"], d["test_data"], m, n, f,
                          r.nnz, r.nnz_test, lam, 5, kw.pop("xb", 1), kw.pop("tb", 1), 0, thetat_init=th0,
                          xt_init=x0, return_log=True, **kw)

    for solver in ("cg", "lu"):
        th_o, x_o = th0.copy(), x0.copy()
        rm_o, log_o = oracle.do_als(d, th_o, x_o, m, n, f, lam, 5, solver=solver)
        th64, x64 = th0.copy(), x0.copy()
        rm_64, log_64 = oracle.do_als(d, th64, x64, m, n, f, lam, 5, solver=solver, dtype=np.float64)
        th, x, rm, log = run(solver=solver)
        if solver == "lu":
            assert np.abs(th - th_o).max() <= 1e-4 * np.abs(th_o).max()
            assert np.abs(x - x_o).max() <= 1e-4 * np.abs(x_o).max()
            assert np.abs(log - log_o).max() <= 1e-5
        else:
            floor = np.abs(log_64 - log_o).max()
            tol = 1e-4 if nnz >= 40000 else max(1e-4, floor)
            assert np.abs(log - log_o).max() <= tol, (np.abs(log - log_o).max(), floor)
            assert abs(rm - rm_o) <= tol
        # batches change nothing (als.cu:768-777)
        th2, x2, rm2, _ = run(solver=solver, xb=3, tb=2)
        np.testing.assert_array_equal(th2, th)
        np.testing.assert_array_equal(x2, x)
        # unfused (reference data flow: Gram batch in HBM + separate solver) agrees with fused
        th3, x3, rm3, _ = run(solver=solver, fused=False)
        # (CG on the under-determined set: the unfused path may run another Gram arithmetic than the
        # fused one -- split materialise vs fp32-MFMA fused CG -- so the bound is the oracle's own
        # fp32-vs-fp64 spread there, as above)
        assert abs(rm3 - rm) <= (1e-5 if solver == "lu" else tol)


@pytest.mark.parametrize("gram_mode", ["exact", "auto"], indirect=True)
@pytest.mark.parametrize("f", [20, 100, 200])
def test_fp16_gram_storage(oracle, alslib, gram_mode, f):
    """CUMF_TT_FP16.  get_hermitian100_tt_fp16 (als.cu:335-441) accumulates in fp32 and
    stores __float2half_rn(value); updateXWithCGKernel3 (cg.cu:235-429) is the fp32 CG reading halves.
    Oracle variant: the oracle's Gram rounded through numpy float16 (IEEE round-to-nearest-even, the
    same rounding) + the oracle's CG on the widened matrix."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(64, 90, 2500, 300, seed=8)
    d = r.numpy()
    theta = _factors(r.n, f, 3)
    lam = 0.05
    A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam)
    A16 = A.astype(np.float16)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), lam, half=True)
    torch.cuda.synchronize()
    assert tt.dtype == torch.float16
    got = tt.cpu().numpy()
    if gram_mode == "exact":
        np.testing.assert_array_equal(got, A16)          # same fp32 chain, same rounding
        np.testing.assert_array_equal(rhs.cpu().numpy(), b)
    else:                                                 # split Gram: fp32-class differences may flip a half ulp
        assert np.abs(got.astype(np.float32) - A16.astype(np.float32)).max() <= 1e-3 * np.abs(A).max()
        assert (got != A16).mean() <= 2e-3
    # CG on the fp16 matrix actually stored on the device
    x0 = _factors(r.m, f, 9) * 0.1
    x_o = oracle.cg(got.astype(np.float32), x0, b, f, 6)
    x = torch.from_numpy(x0.copy()).cuda()
    als.cg_solve(tt, x, rhs, 6)
    torch.cuda.synchronize()
    if f <= 100:
        err = np.abs(x.cpu().numpy() - x_o).max()
        assert err <= 2e-4 * max(1.0, np.abs(x_o).max()), err
    # residual form of the tolerance; at f = 200 the 39-rating rows are under-determined
    # and the half-rounded Gram is barely definite: the truncated CG iterates differ in x but must be
    # equally good solutions
    A64, b64 = got.astype(np.float64), b.astype(np.float64)
    res_h = np.linalg.norm(np.einsum("bij,bj->bi", A64, x.cpu().numpy().astype(np.float64)) - b64, axis=1)
    res_o = np.linalg.norm(np.einsum("bij,bj->bi", A64, x_o.astype(np.float64)) - b64, axis=1)
    assert (np.abs(res_h - res_o) <= 2e-3 * np.linalg.norm(b64, axis=1)).all(), np.abs(res_h - res_o).max()


def test_doals_tt_fp16(oracle, alslib):
    """doALS with CUMF_TT_FP16 semantics end to end (2 iterations, CG) against a restatement built from
    the oracle's pieces: Gram -> float16 round trip -> CG, X side then Theta side (als.cu:727-964)."""
    _need_gpu()
    from cumf_als_amd import als

    m, n, nnz, nnz_test, f, lam = 300, 200, 30000, 2000, 20, 0.05
    r = _dataset(m, n, nnz, nnz_test, seed=4)
    d = r.numpy()
    th0, x0 = oracle.init_factors(m, n, f)
    th, x = th0.copy(), x0.copy()
    for _ in range(2):
        A, b = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], th, f, lam)
        x = oracle.cg(A.astype(np.float16).astype(np.float32), x, b, f, 6)
        A, b = oracle.gram_rhs(d["csc_indptr"], d["csc_indices"], d["csc_data"], x, f, lam)
        th = oracle.cg(A.astype(np.float16).astype(np.float32), th, b, f, 6)
    rm_ref = np.sqrt(oracle.sse(d["test_data"], d["test_row"], d["test_col"], th, x, r.nnz_test, f) / r.nnz_test)
    # bit-exact Gram arithmetic: the device stores the same halves as the restatement above; with the split
    # Gram a few per mille of the halves differ by an ulp and the truncated CG amplifies that (RMSE still
    # agrees: checked below)
    als.set_gram_mode("exact")
    th_h, x_h, rm, log = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"],
                                    d["csc_indptr"], d["csc_data"], d["coo_row"], d["test_row"], d["test_col"],
                                    d["test_data"], m, n, f, r.nnz, r.nnz_test, lam, 2, 1, 1, 0, thetat_init=th0,
                                    xt_init=x0, solver="cg", exact_test_grid=True, return_log=True, tt_fp16=True)
    als.set_gram_mode("auto")
    # tolerance: the stored halves carry 5e-4 relative rounding and the threshold-stopped CG amplifies
    # summation-order differences on such matrices: RMSE 5e-4, factors 5e-2 of their scale
    assert abs(rm - rm_ref) <= 5e-4, (rm, rm_ref)
    assert np.abs(th_h - th).max() <= 5e-2 * np.abs(th).max()
    _, _, rm_split, _ = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"],
                                   d["csc_indptr"], d["csc_data"], d["coo_row"], d["test_row"], d["test_col"],
                                   d["test_data"], m, n, f, r.nnz, r.nnz_test, lam, 2, 1, 1, 0, thetat_init=th0,
                                   xt_init=x0, solver="cg", exact_test_grid=True, return_log=True, tt_fp16=True)
    assert abs(rm_split - rm_ref) <= 2e-3, (rm_split, rm_ref)
    # and it is a different algorithm from the fp32 path (the switch is live)
    th32, x32, rm32, _ = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"],
                                    d["csc_indptr"], d["csc_data"], d["coo_row"], d["test_row"], d["test_col"],
                                    d["test_data"], m, n, f, r.nnz, r.nnz_test, lam, 2, 1, 1, 0, thetat_init=th0,
                                    xt_init=x0, solver="cg", exact_test_grid=True, return_log=True)
    assert not np.array_equal(th32, th_h)


@pytest.mark.parametrize("solver", ["lu", "cg"])
@pytest.mark.parametrize("f", [100, 96, 64, 20])
def test_fused_train_sse_matches_the_rmse_kernel(oracle, alslib, f, solver):
    """Round 4: the Theta update delivers the train SSE of its columns from the systems it has just solved
    (cumf_als_update_fused_sse: entry (f, f) of the augmented Gram -- sum r^2 -- turned into its Schur complement by
    the LU, or S - x.b - x.r - reg |x|^2 after the CG; no rating or factor row read again).  Against the RMSE kernel
    (als.cu:191-219 restated, cumf_sse) and the oracle's fp64 sum on the same factors: relative 2e-5 (it is an
    identity; what differs is where fp32 rounding happens -- measured 1e-7 .. 3e-6)."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(900, 700, 60000, 500, seed=5)
    d = r.numpy()
    rg = r.to("cuda")
    eng = als.ALSEngine(rg, f, 0.05, solver=solver)
    eng.init_factors(_factors(r.n, f, 3))
    for it in range(3):
        eng.update_x()
        fused = eng.update_theta_with_train_sse()
        assert fused is not None
        torch.cuda.synchronize()
        kern = float(als.sse(rg.csr_data, rg.coo_row, rg.csr_indices, eng.thetaT, eng.XT).item())
        ref = oracle.sse(d["csr_data"], d["coo_row"], d["csr_indices"], eng.thetaT.cpu().numpy(), eng.XT.cpu().numpy(),
                         r.nnz, f, dtype=np.float64)
        got = float(fused.item())
        print(f"fused train SSE f={f} {solver} iter {it}: fused {got:.6f} kernel {kern:.6f} oracle64 {ref:.6f}  "
              f"rel {abs(got - kern) / kern:.2e} / {abs(got - ref) / ref:.2e}")
        assert abs(got - kern) <= 2e-5 * kern and abs(got - ref) <= 2e-5 * ref, (got, kern, ref)


def test_doals_rmse_log_fused_vs_kernel(alslib):
    """doALS with the train RMSE taken from the Theta update (default) and from the RMSE kernel (CUMF_ALS_RMSE=kernel,
    the reference's data flow als.cu:966-991): the logs agree to 2e-6 and the factors are bit-identical (the fused SSE
    only reads what the solver leaves behind)."""
    _need_gpu()
    import os

    from cumf_als_amd import als

    m, n, nnz, nnz_test, f, lam = 1200, 900, 90000, 4000, 100, 0.05
    r = _dataset(m, n, nnz, nnz_test, seed=8)
    d = r.numpy()
    th0 = _factors(n, f, 2)

    def run(solver):
        return als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"], d["csc_data"],
                          d["coo_row"], d["test_row"], d["test_col"], d["test_data"], m, n, f, r.nnz, r.nnz_test, lam, 4, 1, 2,
                          0, thetat_init=th0, solver=solver, return_log=True)

    for solver in ("lu", "cg"):
        th_a, x_a, rm_a, log_a = run(solver)
        os.environ["CUMF_ALS_RMSE"] = "kernel"
        try:
            th_b, x_b, rm_b, log_b = run(solver)
        finally:
            del os.environ["CUMF_ALS_RMSE"]
        np.testing.assert_array_equal(th_a, th_b)
        np.testing.assert_array_equal(x_a, x_b)
        print(f"doALS {solver}: fused log {log_a[:, 0].tolist()} kernel log {log_b[:, 0].tolist()}")
        assert np.abs(log_a - log_b).max() <= 2e-6 * max(1.0, np.abs(log_b).max()), (log_a, log_b)
        assert rm_a == rm_b


def test_doals_fused_rmse_near_perfect_fit_is_reevaluated(alslib):
    """the fused train SSE is sum r^2 - 2 t.b + t^T G t in fp32 -- fine while the fit leaves a few per cent of
    sum r^2, mostly cancellation noise when the fit is near-perfect.  doALS takes sum r^2 once and hands an iteration whose
    fused SSE falls below 1e-3 of it to the RMSE kernel: on noise-free rank-4 ratings with a tiny lambda every logged train
    RMSE must agree with the all-kernel run (CUMF_ALS_RMSE=kernel) to 2e-4 RELATIVE although the last ones are below 1e-2
    of the ratings' rms."""
    _need_gpu()
    import os

    from cumf_als_amd import als, datagen

    m, n, nnz, nnz_test, f, lam = 600, 500, 60000, 2000, 16, 1e-7
    rng = np.random.RandomState(3)
    cells = rng.choice(m * n, nnz + nnz_test, replace=False)
    rows, cols = cells // n, cells % n
    xs, ts = rng.uniform(0.5, 1.5, (m, 4)), rng.uniform(0.5, 1.5, (n, 4))
    vals = (xs[rows] * ts[cols]).sum(1).astype(np.float32)          # exactly rank 4, no noise, not quantised
    r = datagen.from_coo(m, n, rows[:nnz], cols[:nnz], vals[:nnz], rows[nnz:], cols[nnz:], vals[nnz:])
    d = r.numpy()
    th0 = _factors(n, f, 2)

    def run():
        return als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"], d["csc_data"],
                          d["coo_row"], d["test_row"], d["test_col"], d["test_data"], m, n, f, r.nnz, r.nnz_test, lam, 8, 1, 1,
                          0, thetat_init=th0, solver="lu", return_log=True)

    th_a, x_a, _, log_a = run()
    os.environ["CUMF_ALS_RMSE"] = "kernel"
    try:
        th_b, x_b, _, log_b = run()
    finally:
        del os.environ["CUMF_ALS_RMSE"]
    np.testing.assert_array_equal(th_a, th_b)
    rms_rating = float(np.sqrt((d["csr_data"].astype(np.float64) ** 2).mean()))
    print(f"near-perfect fit: rms rating {rms_rating:.4f}  fused log {log_a[:, 0].tolist()}  kernel log {log_b[:, 0].tolist()}")
    assert log_b[-1, 0] <= 1e-2 * rms_rating, log_b        # the regime the fall-back exists for: SSE < 1e-4 sum r^2
    assert (np.abs(log_a[:, 0] - log_b[:, 0]) <= 2e-4 * log_b[:, 0] + 1e-7).all(), (log_a, log_b)


def test_few_chunked_rows_take_the_split_launch(oracle, alslib):
    """a plan with a few chunked rows among many whole rows (a Theta side with a handful of very long
    columns) launches its chunk items apart from the whole rows, which keep the LU instance without the dump exit.
    Results against the oracle, and bit-identical to the same rows solved from a plan that has no chunked row at all."""
    _need_gpu()
    from cumf_als_amd import als

    f, lam = 100, 0.05
    rng = np.random.RandomState(3)
    n_rows, n_cols = 600, 5000
    lens = rng.randint(20, 300, size=n_rows)
    lens[7], lens[311] = 4500, 3000                      # two long rows: 9 + 6 chunks of 512
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([rng.choice(n_cols, l, replace=False) for l in lens]).astype(np.int32)
    data = rng.randint(1, 6, size=indptr[-1]).astype(np.float32)
    theta = _factors(n_cols, f, 4)
    x_o = oracle.half_iteration(indptr, indices, data, theta, np.zeros((n_rows, f), np.float32), f, lam, solver="lu")
    ci, cv, th = torch.from_numpy(indices).cuda(), torch.from_numpy(data).cuda(), torch.from_numpy(theta).cuda()
    plan = als.Plan(indptr, f, chunk=512)
    assert plan.n_multi_rows == 2 and plan.n_slots == 15
    x = torch.zeros((n_rows, f), device="cuda")
    als.update_fused(plan, ci, cv, th, x, lam, "lu", 6)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    assert np.abs(xh - x_o).max() <= 1e-4 * np.abs(x_o).max()
    assert als.last_kernel_name().endswith("true>")     # the whole rows ran the instance without the dump exit
    plan_whole = als.Plan(indptr, f, chunk=8192)        # no chunked row: one launch of the same instance
    x2 = torch.zeros((n_rows, f), device="cuda")
    als.update_fused(plan_whole, ci, cv, th, x2, lam, "lu", 6)
    torch.cuda.synchronize()
    short = np.ones(n_rows, bool)
    short[[7, 311]] = False
    np.testing.assert_array_equal(xh[short], x2.cpu().numpy()[short])


@pytest.mark.parametrize("f", [100, 64])
@pytest.mark.parametrize("lam", [0.05, 1e-3, 1e-5])
def test_fused_lu_on_ill_conditioned_systems(oracle, alslib, f, lam):
    """Round 4: the wave kernels' LU scales its eliminated rows by 1 / sqrt(u_kk) (v_rsq_f32) and runs the trailing
    updates as bf16x3 products; neither may cost accuracy when the regulariser is small and the systems get
    ill-conditioned (condition number ~ |x|^2 / lambda: 1e2 .. 1e6 here; rows with more ratings than features, so that the
    Gram itself is well defined).  Yardstick as at full size: per row, distance from the fp64 evaluation of the same
    half-iteration relative to the row's scale; median / 99th percentile / maximum of the HIP rows no worse than
    2 x the fp32 oracle's (the reference's own unpivoted fp32 LU) + 1e-5."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(400, 3000, 160000, 600, seed=21)     # ~400 ratings per row
    d = r.numpy()
    theta = _factors(r.n, f, 5) - 0.08               # mixed signs
    x0 = np.zeros((r.m, f), np.float32)
    x32 = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam, solver="lu")
    x64 = oracle.half_iteration(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, x0.copy(), f, lam, solver="lu",
                                dtype=np.float64)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    x = torch.from_numpy(x0.copy()).cuda()
    als.update_fused(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), x, lam, "lu", 6)
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    fin = np.isfinite(x64).all(1)
    assert np.array_equal(np.isfinite(xh).all(1), fin)
    den = np.maximum(np.abs(x64[fin]).max(1), 1e-30)
    e_h = np.abs(xh[fin] - x64[fin]).max(1) / den
    e_o = np.abs(x32[fin] - x64[fin]).max(1) / den
    stats = lambda v: (float(np.median(v)), float(np.quantile(v, 0.99)), float(v.max()))
    print(f"ill-conditioned LU f={f} lambda={lam}: per-row relative |x - x64| (median, q99, max): hip {stats(e_h)}  "
          f"oracle32 {stats(e_o)}")
    for sh, so in zip(stats(e_h), stats(e_o)):
        assert sh <= 2.0 * so + 1e-5, (stats(e_h), stats(e_o))


@pytest.mark.parametrize("solver", ["cg", "lu"])
@pytest.mark.parametrize("f,chunk", [(128, 0), (200, 0), (160, 64), (100, 64), (64, 32)])
def test_fused_train_sse_large_f_and_chunked_rows(oracle, alslib, f, chunk, solver):
    """The fused train SSE beyond the one-wave whole-row case.  CG (S - x.b - x.r - reg |x|^2) wherever the wave kernels'
    CG runs: the two-wave kernel (f >= 112: the wave that owns the last diagonal tile reports), chunked rows (partial
    tiles summed by als_wave_cg_kernel, one or four waves).  LU (the Schur complement of slot f) in lu_solve_mfma: two
    wave roles in place (f = 128), four from the tile buffer (f = 200), chunked rows through als_reduce_kernel from
    NB = 7 on -- below that (f = 64 with chunked rows) the thread-grid LU serves and the RMSE kernel is the way.
    Against the RMSE kernel and the oracle's fp64 sum: 2e-5 relative."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(500, 400, 40000, 300, seed=9)
    d = r.numpy()
    rg = r.to("cuda")
    eng = als.ALSEngine(rg, f, 0.05, solver=solver, chunk=chunk)
    eng.init_factors(_factors(r.n, f, 3))
    if chunk:
        assert any(p.n_multi_rows > 0 for p in eng.t_plans)
    expect = not (solver == "lu" and chunk and f < 96)
    assert all(als.fused_sse_available(p, solver) for p in eng.t_plans) == expect
    for it in range(2):
        eng.update_x()
        fused = eng.update_theta_with_train_sse()
        if not expect:
            assert fused is None
            continue
        torch.cuda.synchronize()
        kern = float(als.sse(rg.csr_data, rg.coo_row, rg.csr_indices, eng.thetaT, eng.XT).item())
        ref = oracle.sse(d["csr_data"], d["coo_row"], d["csr_indices"], eng.thetaT.cpu().numpy(), eng.XT.cpu().numpy(),
                         r.nnz, f, dtype=np.float64)
        got = float(fused.item())
        print(f"fused train SSE ({solver}) f={f} chunk={chunk} iter {it}: fused {got:.6f} kernel {kern:.6f} oracle64 {ref:.6f}  "
              f"rel {abs(got - kern) / kern:.2e}")
        assert abs(got - kern) <= 2e-5 * kern and abs(got - ref) <= 2e-5 * ref, (got, kern, ref)


def _presplit_tool():
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("presplit_check", os.path.join(root, "tools", "presplit_check.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("f", [100, 64, 96, 68, 200, 128, 120, 180])
def test_presplit_planes_are_the_in_kernel_split(alslib, f):
    """Round 6 (kArithPre): the pre-split gather table holds, per value, exactly the three bf16 terms the in-kernel split
    produces -- checked against a numpy restatement of the split (round to nearest even, exact residuals) over 17 decades
    of magnitude, and h + m + l == x exactly."""
    _need_gpu()
    o = _presplit_tool().check_planes(f)
    assert o["planes_equal_numpy_split"] and o["h_plus_m_plus_l_exact"], o


@pytest.mark.parametrize("solver", ["lu", "cg"])
@pytest.mark.parametrize("f", [100, 64, 96, 68, 200, 128, 120, 180])
def test_presplit_is_bit_identical(alslib, f, solver):
    """The fused half-iteration from the pre-split table (16-byte LDS-DMA + transposing LDS reads) against the same call with
    the in-kernel split, over rows of 0, 1, 31, 32, 33, ... ratings, a chunked row of 9 000 and 150 random ones: the
    verification form (cumf_set_presplit(CUMF_PRESPLIT_VERIFY): the same operands in the same MFMA K slots) must give the
    factors -- and the fused train SSE bins -- BIT FOR BIT; the production form (last block packed) the same error class."""
    _need_gpu()
    o = _presplit_tool().check_fused(f, solver)
    arith = lambda k: o[k].split(",")[3].strip().rstrip(">")
    # (the two-wave kernels of f >= 112 have the one pre-split form, the bit-identical one)
    assert (arith("kernel_off"), arith("kernel_verify"), arith("kernel_on")) == ("0", "2", "3" if f < 112 else "2"), o
    assert o["bit_identical"] and o["sse_bins_identical"] in (True, None), o
    # the production form multiplies the last feature block as ONE packed operand (three products instead of six, all nine
    # plane products kept): the error class of the in-kernel split, not its bits -- 2e-5 of the factors' scale here (measured
    # 1e-7 .. 3e-6), the fused train SSE to 1e-6; the oracle-level bounds are those of test_fused_half_iteration etc., which
    # run this form wherever the table is small
    assert o["packed_nan_pattern_equal"] and o["packed_max_rel_diff"] < 2e-5, o
    assert o["packed_sse_rel_diff"] is None or o["packed_sse_rel_diff"] < 1e-6, o


@pytest.mark.parametrize("solver", ["lu", "cg"])
@pytest.mark.parametrize("f", [16, 32, 48, 64, 80, 96])
def test_packed_rating_block_matches_six_product_form(alslib, f, solver):
    """Round 6, kArithSplitPk: at f % 16 == 0 the last feature block holds nothing but the rating slot, and the in-kernel split
    multiplies it as ONE packed operand [r_h r_m r_l 0 ...] (three products per tile of its column instead of six, all nine plane
    products of the rating kept; no gather of the block) -- what the library picks by itself ("auto") wherever the table is not
    pre-split.  Against the six-product form (cumf_set_presplit(CUMF_PRESPLIT_OFF)) on rows of 0, 1, 31, 32, 33, ... ratings, a
    chunked row of 9 000 and 150 random ones: same NaN pattern, factors within 2e-5 of their scale (the bound of the packed
    pre-split form; only the right-hand side column and sum r^2 see other roundings), fused train SSE to 1e-6."""
    _need_gpu()
    o = _presplit_tool().check_fused(f, solver, modes=("off", "auto"))
    arith = lambda k: o[k].split(",")[3].strip().rstrip(">")
    assert arith("kernel_off") == "0", o
    # (f = 96 with a small table: "auto" pre-splits it -- the packed pre-split form, the same bound)
    assert arith("kernel_auto") == ("3" if f == 96 else "4"), o
    assert o["packed_nan_pattern_equal"] and o["packed_max_rel_diff"] < 2e-5, o
    assert o["packed_sse_rel_diff"] is None or o["packed_sse_rel_diff"] < 1e-6, o


def test_presplit_auto_follows_the_table_size(alslib, monkeypatch):
    """CUMF_PRESPLIT_AUTO: a table whose planes fit the cache budget (64 MB) takes the pre-split kernels, a larger one (the
    Netflix X side gathers 192 MB of Theta) keeps the fp32 table: there the bytes are the roof."""
    _need_gpu()
    from cumf_als_amd import als

    f = 100
    rng = np.random.RandomState(0)
    lens = rng.randint(1, 200, 64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    plan = als.Plan(indptr, f)
    for n_rows, want in ((5000, "3"), (200000, "0")):   # 3 MB / 122 MB of planes
        idx = torch.from_numpy(rng.randint(0, n_rows, int(indptr[-1])).astype(np.int32)).cuda()
        val = torch.ones(int(indptr[-1]), device="cuda")
        table = torch.rand((n_rows, f), device="cuda")
        x = torch.zeros((len(lens), f), device="cuda")
        als.update_fused(plan, idx, val, table, x, 0.05, "lu", 6)
        torch.cuda.synchronize()
        assert als.last_kernel_name().split(",")[3].strip() == want, (n_rows, als.last_kernel_name())


@pytest.mark.parametrize("f", [250, 210, 320])
def test_generic_gram_and_lu_above_the_tile_range_are_bit_exact(oracle, alslib, f):
    """VERDICT r05 missing 3: the reference's generic kernel takes every f % 10 == 0 (get_hermitianT10, als.cu:575-659;
    `./main ... 250 ...` works there); the tile kernels stop at f = 207.  Above that the plain kernels of als_generic.hip run
    the reference's own data flow in its own operation order: the Gram batch and right-hand sides are one fmaf chain per
    entry over the row's ratings (bit-exact vs the oracle), the unpivoted LU + triangular solves in global memory repeat the
    oracle's operation sequence element by element (bit-exact too); CG(6) on the same systems to the usual tolerance."""
    _need_gpu()
    from cumf_als_amd import als

    r = _dataset(40, 300, 2500, 100, seed=f, row_alpha=1.2)
    d = r.numpy()
    theta = _factors(r.n, f, 1)
    lam = 0.05
    tt_o, b_o = oracle.gram_rhs(d["csr_indptr"], d["csr_indices"], d["csr_data"], theta, f, lam)
    rg = r.to("cuda")
    plan = als.Plan(d["csr_indptr"], f)
    assert plan.n_multi_rows == 0 and plan.n_items == r.m
    tt, rhs = als.get_hermitian(plan, rg.csr_indices, rg.csr_data, torch.from_numpy(theta).cuda(), lam)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tt.cpu().numpy(), tt_o)
    np.testing.assert_array_equal(rhs.cpu().numpy(), b_o)
    keep = np.diff(d["csr_indptr"]) > 0          # an all-zero system (a row without ratings) is 0 / 0 in both
    x_o = oracle.lu(tt_o.copy(), b_o.copy(), f)
    x = als.lu_solve(tt.clone(), rhs).cpu().numpy()
    np.testing.assert_array_equal(x[keep], x_o[keep])
    assert np.isnan(x[~keep]).all() and np.isnan(x_o[~keep]).all()
    x0 = np.zeros_like(b_o)
    xc_o = oracle.cg(tt_o, x0.copy(), b_o, f, 6)
    xc = als.cg_solve(tt, torch.zeros_like(rhs), rhs, 6).cpu().numpy()
    # rows with far fewer ratings than features: six truncated iterations are sensitive element-wise (f = 320: the fp32 oracle
    # itself leaves its fp64 evaluation by 3e-4), so the bound lives on the residual as in test_fused_half_iteration: the HIP
    # iterate solves its system as well as the oracle's does, ||A x - b|| within 1e-4 ||b|| per system; element-wise 2e-3
    A64, b64 = tt_o.astype(np.float64), b_o.astype(np.float64)
    res = lambda xx: np.linalg.norm(np.einsum("bij,bj->bi", A64, xx.astype(np.float64)) - b64, axis=1)
    r_h, r_o, nb_ = res(xc), res(xc_o), np.linalg.norm(b64, axis=1)
    assert (np.abs(r_h - r_o)[keep] <= 1e-4 * nb_[keep] + 1e-6).all(), np.abs(r_h - r_o)[keep].max()
    assert np.abs(xc[keep] - xc_o[keep]).max() <= 2e-3 * max(1.0, np.abs(xc_o[keep]).max())


@pytest.mark.parametrize("solver", ["lu", "cg"])
def test_doals_at_f_250(oracle, alslib, solver):
    """doALS at f = 250 (the reference's CLI accepts it, main.cpp:32-36) against oracle_doALS on a tiny shape: the unfused
    data flow on the plain kernels, X_BATCH = 1 / THETA_BATCH = 2."""
    _need_gpu()
    from cumf_als_amd import als

    # (CG: lambda = 0.5 keeps the 250 x 250 systems of ~20 ratings well conditioned, so that six iterations converge and two
    # implementations of the truncated recurrence can be compared element-wise)
    m, n, f, lam, iters = 30, 40, 250, (0.05 if solver == "lu" else 0.5), 2
    r = _dataset(m, n, 600, 80, seed=5, row_alpha=1.1)
    d = r.numpy()
    th0, x0 = oracle.init_factors(m, n, f)
    th, x, rm, log = als.do_als(d["csr_indptr"], d["csr_indices"], d["csr_data"], d["csc_indices"], d["csc_indptr"],
                                d["csc_data"], d["coo_row"], d["test_row"], d["test_col"], d["test_data"], m, n, f, r.nnz,
                                r.nnz_test, lam, iters, 1, 2, 0, thetat_init=th0, xt_init=x0, solver=solver, cg_iters=6,
                                return_log=True)
    th_o, x_o = th0.copy(), x0.copy()
    rm_o, log_o = oracle.do_als(d, th_o, x_o, m, n, f, lam, iters, x_batch=1, theta_batch=2, solver=solver, cg_iters=6)
    assert np.abs(np.asarray(log) - np.asarray(log_o)).max() <= 1e-4, (log, log_o)
    fin = np.isfinite(th_o.reshape(n, f))
    tol = 1e-4 if solver == "lu" else 2e-3
    assert np.abs(th.reshape(n, f)[fin] - th_o.reshape(n, f)[fin]).max() <= tol * np.abs(th_o[np.isfinite(th_o)]).max()
