"""The range guard of the opt-in gram mode "fast" (presplit_f16x2_kernel of als_common.hip) at its seams.  The guard is the only
thing between data outside the f16 range of the pre-split words and silently wrong factors: it scans the WHOLE gather table
of a fused call -- 16 bytes per thread while the table is 16-byte aligned, the elements 4 (n / 4) .. n - 1 in a scalar tail,
everything in that scalar loop when the table is not aligned, grid-stride beyond 4096 x 256 threads -- and reports
|x| * 4096 >= 65504 (+-inf included, NaN not) in bit 0 of als.gram_fast_status().

The plan is tiny: 8 rows of 40 ratings on table rows 1 .. 63, so row 0 and every row from 64 on are never gathered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAM = 0.05
EDGE = np.float32(15.9921875)          # 65504 / 4096: the first magnitude whose scaled value leaves the finite f16 range
BELOW = np.nextafter(EDGE, np.float32(0))


def _plan_data():
    indptr = (40 * np.arange(9)).astype(np.int32)
    indices = np.concatenate([np.sort(1 + (7 * u + np.arange(40)) % 63) for u in range(8)]).astype(np.int32)
    data = np.random.RandomState(0).randint(1, 6, len(indices)).astype(np.float32)
    assert indices.min() == 1 and indices.max() == 63 and 5 in indices[:40]
    return indptr, indices, data


def _table(rows, f, seed=1):
    return (0.2 * np.random.RandomState(seed).random_sample((rows, f))).astype(np.float32)


class _Fast:
    """Gram mode "fast" for the length of a `with`, the flags cleared on entry; the mode is restored on exit."""

    def __init__(self, f):
        from cumf_als_amd import als

        self.als, self.f = als, f
        self.indptr, indices, data = _plan_data()
        self.indices, self.data = torch.from_numpy(indices).cuda(), torch.from_numpy(data).cuda()
        self.host = (indices, data)

    def __enter__(self):
        self.als.set_gram_mode("fast")
        self.als.gram_fast_status()
        self.plan = self.als.Plan(self.indptr, self.f)
        return self

    def __exit__(self, *exc):
        self.plan.close()
        self.als.gram_fast_status()
        self.als.set_gram_mode("auto")

    def update(self, table, mode="fast"):
        """(factors of the 8 rows, status) of one LU half-iteration over `table` (a device tensor or a numpy array)."""
        if not torch.is_tensor(table):
            table = torch.from_numpy(np.ascontiguousarray(table)).cuda()
        assert table.shape[1] == self.f
        self.als.set_gram_mode(mode)
        try:
            self.als.gram_fast_status()  # a read clears
            x = torch.zeros((8, self.f), device="cuda")
            self.als.update_fused(self.plan, self.indices, self.data, table, x, LAM, "lu", 6)
            torch.cuda.synchronize()
            return x.cpu().numpy(), self.als.gram_fast_status()
        finally:
            self.als.set_gram_mode("fast")


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_threshold(oracle, alslib, sign):
    """The threshold itself, f = 32, the value in a gathered row: the largest fp32 below 65504 / 4096 passes -- status 0, finite
    factors within the bound of test_fast_gram_error_class of the fp64 solution (1e-5 relative, and 4 x the distance of the
    default arithmetic + 1e-6) -- while 65504 / 4096 itself and +-inf set bit 0, which the next read finds cleared.  A NaN
    in a row that no rating gathers is not a range violation."""
    f = 32
    with _Fast(f) as g:
        indices, data = g.host
        base = _table(65, f)
        ok = base.copy()
        ok[5, 3] = sign * BELOW
        assert abs(ok[5, 3]) < EDGE and abs(ok[5, 3]) * np.float32(4096.0) < 65504.0
        tt64, b64 = oracle.gram_rhs(g.indptr, indices, data, ok, f, LAM, dtype=np.float64)
        x64 = np.linalg.solve(tt64, b64[..., None])[..., 0]
        err = {}
        for mode in ("auto", "fast"):
            x, status = g.update(ok, mode)
            assert status == 0 and np.isfinite(x).all(), (mode, status)
            err[mode] = np.abs(x - x64).max() / np.abs(x64).max()
        print(f"fast guard threshold sign = {sign:+.0f}: distance to fp64 {err}")
        assert err["fast"] <= 1e-5, err
        assert err["fast"] <= 4 * err["auto"] + 1e-6, err
        for v in (sign * EDGE, sign * np.float32(np.inf)):
            bad = base.copy()
            bad[5, 3] = v
            _, status = g.update(bad)
            assert status & 1, (v, status)
            assert g.als.gram_fast_status() == 0
        nan = base.copy()
        nan[64, 3] = np.nan
        nan[0] = np.nan
        x, status = g.update(nan)
        assert status == 0 and np.isfinite(x).all()


@pytest.mark.parametrize("where", ["0", "3", "4", "last_vector", "n-2", "n-1"])
def test_placement(alslib, where):
    """f = 18 with 65 table rows: n = 1170 elements, n % 4 = 2, so 292 threads take 16 bytes each and the scalar tail takes
    the last two.  40.0 at the first and the last element of the first vector, the first of the second, the last
    element of the last vector and both tail elements -- all in rows that no rating gathers -- sets bit 0 every time."""
    f, rows = 18, 65
    n = rows * f
    assert n == 1170 and n % 4 == 2
    at = {"0": 0, "3": 3, "4": 4, "last_vector": 4 * (n // 4) - 1, "n-2": n - 2, "n-1": n - 1}[where]
    assert at // f in (0, 64)
    with _Fast(f) as g:
        clean = _table(rows, f)
        x0, status = g.update(clean)
        assert status == 0 and np.isfinite(x0).all()
        bad = clean.copy()
        bad.reshape(-1)[at] = 40.0
        x, status = g.update(bad)
        assert status & 1, (where, status)
        np.testing.assert_array_equal(x, x0)   # the row is not gathered: the factors do not see it
        assert g.als.gram_fast_status() == 0


def test_unaligned_table(alslib):
    """The same 65 x 18 table as rows 1 .. 65 of a 66 x 18 tensor: 72 bytes into the allocation, not 16-byte aligned, so the
    whole table goes through the scalar loop (n4 = 0).  Clean data: bit-identical factors to an aligned copy; 40.0 at the
    last element: bit 0."""
    f, rows = 18, 65
    with _Fast(f) as g:
        big = torch.zeros((rows + 1, f), device="cuda")
        view = big[1:]
        view.copy_(torch.from_numpy(_table(rows, f)))
        assert view.is_contiguous() and big.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8
        aligned = view.clone()
        assert aligned.data_ptr() % 16 == 0
        x_a, status = g.update(aligned)
        assert status == 0
        x_u, status = g.update(view)
        assert status == 0 and np.isfinite(x_u).all()
        np.testing.assert_array_equal(x_u, x_a)
        view[rows - 1, f - 1] = 40.0
        _, status = g.update(view)
        assert status & 1
        assert g.als.gram_fast_status() == 0


def test_second_grid_trip(alslib):
    """f = 64 with 65 600 table rows: 4 198 400 elements, 1 049 600 vectors for 4096 x 256 = 1 048 576 threads, so the last
    1024 vectors are a second grid-stride trip.  40.0 at the last element sets bit 0; the clean table gives 0."""
    f, rows = 64, 65600
    assert rows * f // 4 > 4096 * 256
    with _Fast(f) as g:
        gen = torch.Generator(device="cpu").manual_seed(3)
        table = (0.2 * torch.rand((rows, f), generator=gen)).cuda()
        x0, status = g.update(table)
        assert status == 0 and np.isfinite(x0).all()
        table[rows - 1, f - 1] = 40.0
        x, status = g.update(table)
        assert status & 1
        np.testing.assert_array_equal(x, x0)
        assert g.als.gram_fast_status() == 0
        table[rows - 1, f - 1] = 0.1
        table[1024 * 1024 * 4 // f, 0] = 40.0   # the first element of the second trip
        _, status = g.update(table)
        assert status & 1
    g.als.release_scratch()
