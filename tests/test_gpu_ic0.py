"""ic0_csr (include/spmv/ic0.h) on the GPU: the device factor against ic0_cpu_csr at zero tolerance for every lane
count, out of place and in place, over shapes that reach both launch kinds, the 8192-level split, a row longer than
64 * 4 entries whose mirror stores land in every other row; the schedule cache; the async entry on a side stream; an
output that is a view into a larger buffer; rejection before d_l_values is written; the reported bad pivot; and the
factor put to use by two sptrsv_csr calls."""
import ctypes
import importlib

import numpy as np
import pytest

import ic0_cases as cases
from test_ic0_host import REJECTED

pytestmark = pytest.mark.gpu

LANES = (1, 2, 4, 8, 16, 32, 64)
NARROW = 256          # csrc/internal.h kSptrsvNarrowRows
MAX_RUN = 8192        # csrc/internal.h kSptrsvMaxRunLevels

spd = importlib.import_module("gpu-spmv_amd.spd")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _upload(gpu, n, rp, ci, va):
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    return A


def _download(gpu, address, count):
    out = np.empty(count, np.float32)
    assert gpu.lib().spmv_c_memcpy_d2h(_ptr(out), ctypes.c_void_p(address), out.nbytes) == 0
    return out


def _restore(gpu, A, va):
    va = np.ascontiguousarray(va, np.float32)
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(A.contents.d_values), _ptr(va), va.nbytes) == 0


def _factor(gpu, A, va, in_place, sentinel=np.nan):
    """(result, l values); in place factors A's own device values and puts A's values back afterwards"""
    nnz = int(A.contents.nnz)
    if in_place:
        res = gpu.ic0_csr(A, A.contents.d_values)
        l = _download(gpu, A.contents.d_values, nnz)
        _restore(gpu, A, va)
        return res, l
    d_l = gpu.CudaBuffer(max(nnz, 1))
    d_l.copyFromHost(np.full(max(nnz, 1), sentinel, np.float32), max(nnz, 1))
    res = gpu.ic0_csr(A, d_l)
    l = d_l.copyToHost(max(nnz, 1))[:nnz]
    d_l.release()
    return res, l


SHAPES = {
    "exact_tridiagonal(257)": lambda: cases.exact_tridiagonal(257)[:4],
    "exact_tridiagonal(8200)": lambda: cases.exact_tridiagonal(8200)[:4],
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "spd_blocks(300)": lambda: cases.spd_blocks(300),
    "arrow_spd(600)": lambda: cases.arrow_spd(600),
    "sorted_random_spd(2000,8)": lambda: cases.sorted_random_spd(2000, 8, 11),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_factor_equals_the_cpu_bit_for_bit_at_every_lane_count(gpu, monkeypatch, name):
    n, rp, ci, va = SHAPES[name]()
    A = _upload(gpu, n, rp, ci, va)
    want, want_pivot = gpu.ic0_cpu_csr(A)
    assert want_pivot == -1
    _, level_ptr, _, levels, _ = gpu.sptrsv_levels(n, rp, ci, 0)
    widths = np.diff(level_ptr)
    launches = None
    # what the shape is here for
    if name.startswith("exact_tridiagonal"):
        fact = cases.exact_tridiagonal(n)[4]
        np.testing.assert_array_equal(_bits(cases.prove_exact(n, rp, ci, va)), _bits(fact))
        np.testing.assert_array_equal(_bits(want), _bits(fact))
        assert levels == n
        launches = 2 if n > MAX_RUN else 1
    elif name.startswith("arrow"):
        np.testing.assert_array_equal(_bits(want), _bits(cases.prove_exact(n, rp, ci, va, shift=6)))
        assert widths.tolist() == [n - 1, 1] and np.diff(rp).max() == n > 64 * 4 and np.bincount(ci).max() == n
        launches = 2
    elif name.startswith("poisson2d"):
        assert widths.max() <= NARROW and levels > 1
        launches = 1
    elif name.startswith("spd_blocks"):
        assert widths.tolist() == [300, 300, 300]
        launches = 3
    else:
        assert levels > 3 and np.diff(rp).max() > 8
    try:
        for lanes in LANES + (None,):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"ic0_lanes={lanes}")
            for in_place in (False, True):
                res, got = _factor(gpu, A, va, in_place)
                tag = f"{name} lanes={lanes} in_place={in_place}"
                assert res.error_code == 0 and res.bad_pivot == -1 and res.num_levels == levels, tag
                assert res.lanes_per_row == (lanes if lanes is not None else res.lanes_per_row), tag
                assert res.lanes_per_row in LANES, tag
                if launches is not None:
                    assert res.launches == launches, tag
                assert 1 <= res.launches <= levels, tag
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=tag)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


def test_a_forced_lane_count_that_is_no_lane_count_is_ignored(gpu, monkeypatch):
    """SPMV_DEBUG=ic0_lanes=v with v outside 1, 2, 4, ... 64 changes nothing: the library's own pick, the CPU's bits."""
    n, rp, ci, va = spd.poisson2d(8)
    assert n == 64
    A = _upload(gpu, n, rp, ci, va)
    want, _ = gpu.ic0_cpu_csr(A)
    try:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        own, got = _factor(gpu, A, va, False)
        assert own.error_code == 0 and own.lanes_per_row in LANES
        np.testing.assert_array_equal(_bits(got), _bits(want))
        for value in (0, 3, 128, -4):
            monkeypatch.setenv("SPMV_DEBUG", f"ic0_lanes={value}")
            res, got = _factor(gpu, A, va, False)
            assert res.error_code == 0 and res.lanes_per_row == own.lanes_per_row, value
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(value))
        for lanes in (1, 64):                    # the ends of the range are taken
            monkeypatch.setenv("SPMV_DEBUG", f"ic0_lanes={lanes}")
            res, got = _factor(gpu, A, va, False)
            assert res.error_code == 0 and res.lanes_per_row == lanes
            np.testing.assert_array_equal(_bits(got), _bits(want))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


def test_schedule_cache_the_async_entry_and_an_output_view(gpu):
    import torch
    n, rp, ci, va = spd.poisson3d(12)
    A = _upload(gpu, n, rp, ci, va)
    want, _ = gpu.ic0_cpu_csr(A)
    first, l0 = _factor(gpu, A, va, False)
    assert first.error_code == 0 and first.analysis_ms > 0 and first.elapsed_ms > 0
    second, l1 = _factor(gpu, A, va, False)
    assert second.analysis_ms == 0
    assert (second.num_levels, second.launches, second.lanes_per_row) == (first.num_levels, first.launches,
                                                                         first.lanes_per_row)
    np.testing.assert_array_equal(_bits(l0), _bits(want))
    np.testing.assert_array_equal(_bits(l1), _bits(want))
    # the schedule is sptrsv_csr's LOWER one: already there for a solve, and the other way round
    assert gpu.sptrsv_analyze(A, 0).analysis_ms == 0
    gpu.csr_invalidate_gpu_cache(A)
    assert gpu.sptrsv_analyze(A, 0).analysis_ms > 0 and _factor(gpu, A, va, False)[0].analysis_ms == 0
    # a side stream, out of place and in place
    stream = torch.cuda.Stream()
    out = torch.full((ci.size,), float("nan"), device="cuda")
    own = torch.from_numpy(va).cuda()
    W = gpu.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, own.data_ptr())
    torch.cuda.synchronize()
    assert gpu.ic0_csr_async(A, out.data_ptr(), stream.cuda_stream) == 0
    assert gpu.ic0_csr_async(W, own.data_ptr(), stream.cuda_stream) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(own.cpu().numpy()), _bits(want))
    gpu.csr_destroy(W)
    # the output as a view into a larger buffer: the guard words on both sides stay as they were
    guard = 37
    big = torch.full((ci.size + 2 * guard,), -77.0, device="cuda")
    torch.cuda.synchronize()
    res = gpu.ic0_csr(A, big.data_ptr() + 4 * guard)
    assert res.error_code == 0
    host = big.cpu().numpy()
    np.testing.assert_array_equal(_bits(host[guard:-guard]), _bits(want))
    assert (host[:guard] == -77.0).all() and (host[-guard:] == -77.0).all()
    gpu.csr_destroy(A)


def test_rejections_leave_the_output_untouched(gpu):
    E = gpu.SpMVError
    for name, (rows, ptr, col, val, code) in REJECTED.items():
        code = getattr(E, code)
        val = np.asarray(val, np.float32)
        A = _upload(gpu, rows, ptr, col, val)
        res, l = _factor(gpu, A, val, False, sentinel=-77.0)
        assert res.error_code == code and (l == -77.0).all(), name
        assert gpu.ic0_csr(A, A.contents.d_values).error_code == code, name            # in place: A's values stay
        np.testing.assert_array_equal(_bits(_download(gpu, A.contents.d_values, len(val))), _bits(val), err_msg=name)
        d_l = gpu.CudaBuffer(len(val))
        d_l.copyFromHost(np.full(len(val), -77.0, np.float32), len(val))
        assert gpu.ic0_csr_async(A, d_l, None) == code, name
        assert (d_l.copyToHost(len(val)) == -77.0).all(), name
        # a second call re-checks nothing and answers the same
        assert gpu.ic0_csr(A, d_l).error_code == code and (d_l.copyToHost(len(val)) == -77.0).all(), name
        d_l.release()
        gpu.csr_destroy(A)
    # not square
    R = gpu.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], np.asarray([4, 4], np.float32))
    assert gpu.csr_to_gpu(R) == 0
    res, l = _factor(gpu, R, None, False, sentinel=-77.0)
    assert res.error_code == E.INVALID_DIMENSION and (l == -77.0).all()
    gpu.csr_destroy(R)
    # a one-sided entry far down a larger matrix; a partial overlap with A's device values
    n, rp, ci, va = spd.poisson2d(8)
    keep = np.ones(ci.size, bool)
    keep[np.flatnonzero((cases.rows_of(n, rp) == 40) & (ci == 48))] = False
    lop = cases.csr_from_coo(n, cases.rows_of(n, rp)[keep], ci[keep], va[keep])
    A = _upload(gpu, *lop)
    res, l = _factor(gpu, A, lop[3], False, sentinel=-77.0)
    assert res.error_code == E.INVALID_ARGUMENT and (l == -77.0).all()
    assert gpu.ilu0_csr(A, A.contents.d_values).error_code == 0       # ILU(0) takes the same matrix: not symmetric is fine there
    gpu.csr_destroy(A)
    A = _upload(gpu, n, rp, ci, va)
    assert gpu.ic0_csr(A, A.contents.d_values + 4).error_code == E.INVALID_ARGUMENT
    np.testing.assert_array_equal(_bits(_download(gpu, A.contents.d_values, ci.size)), _bits(va))
    gpu.csr_destroy(A)


def test_bad_pivot_is_reported_like_the_cpu(gpu, monkeypatch):
    dense_cases = {
        "indefinite at row 2": ([[4, 1, 1, 0], [1, 4, 1, 0], [1, 1, .25, 1], [0, 0, 1, 4]], 2),
        "zero pivot at row 1": ([[4, 2, 0], [2, 1, 1], [0, 1, 4]], 1),
        "clean": ([[4, 1, 0], [1, 4, 1], [0, 1, 4]], -1),
    }
    systems = {}
    for name, (dense, want_pivot) in dense_cases.items():
        dense = np.asarray(dense, np.float32)
        rows, cols = np.nonzero(dense)
        systems[name] = (cases.csr_from_coo(dense.shape[0], rows, cols, dense[rows, cols]), want_pivot)
    # rows made indefinite far down a larger matrix: the lowest bad row wins whatever order the scan meets them in
    n, rp, ci, va = spd.poisson3d(12)
    va = va.copy()
    r = cases.rows_of(n, rp)
    for row in (1500, 900, 1300):
        va[(r == row) & (ci == row)] = -6.0
    systems["poisson3d(12), rows 900, 1300, 1500"] = ((n, rp, ci, va), 900)
    for name, ((n, rp, ci, va), want_pivot) in systems.items():
        A = _upload(gpu, n, rp, ci, va)
        want, cpu_pivot = gpu.ic0_cpu_csr(A)
        assert cpu_pivot == want_pivot, name
        for lanes in (1, 4, None):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"ic0_lanes={lanes}")
            for in_place in (False, True):
                res, got = _factor(gpu, A, va, in_place)
                assert (res.error_code, res.bad_pivot) == (0, want_pivot), (name, lanes, in_place)
                np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=name)
                np.testing.assert_array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)], err_msg=name)
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


def test_both_triangular_solves_with_the_factor_header_equal_the_cpu(gpu):
    """LOWER and UPPER NON_UNIT sptrsv_csr (ordered = 1) over csr_wrap_device(A's structure, d_l_values) against
    sptrsv_cpu_csr on the host factor, bit for bit; on the exact factor the two solves are the direct solve."""
    rng = np.random.default_rng(12)
    systems = {"exact_tridiagonal(257)": cases.exact_tridiagonal(257)[:4], "poisson2d(24)": spd.poisson2d(24),
               "sorted_random_spd(2000,8)": cases.sorted_random_spd(2000, 8, 11)}
    for name, (n, rp, ci, va) in systems.items():
        A = _upload(gpu, n, rp, ci, va)
        d_l = gpu.CudaBuffer(ci.size)
        assert gpu.ic0_csr(A, d_l).error_code == 0
        host_l, _ = gpu.ic0_cpu_csr(A)
        np.testing.assert_array_equal(_bits(d_l.copyToHost(ci.size)), _bits(host_l))
        F = gpu.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, d_l.get())
        F_host = gpu.csr_from_arrays(n, n, rp, ci, host_l)
        b = rng.integers(-3, 4, n).astype(np.float32)
        d_b, d_y = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        d_b.copyFromHost(b, n)
        lower, upper = gpu.SpTRSVConfig(uplo=0, diag=0, ordered=1), gpu.SpTRSVConfig(uplo=1, diag=0, ordered=1)
        first = gpu.sptrsv_csr(F, d_b, d_y, lower)
        assert first.error_code == 0 and first.analysis_ms == 0      # the factor shares A's LOWER schedule
        y = d_y.copyToHost(n)
        y_ref = gpu.sptrsv_cpu_csr(F_host, b, lower)
        np.testing.assert_array_equal(_bits(y), _bits(y_ref), err_msg=name)
        assert gpu.sptrsv_csr(F, d_y, d_y, upper).error_code == 0
        x = d_y.copyToHost(n)
        np.testing.assert_array_equal(_bits(x), _bits(gpu.sptrsv_cpu_csr(F_host, y_ref, upper)), err_msg=name)
        assert np.isfinite(x).all()
        for buf in (d_b, d_y, d_l):
            buf.release()
        gpu.csr_destroy(F)
        gpu.csr_destroy(F_host)
        gpu.csr_destroy(A)
