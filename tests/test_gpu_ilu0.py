"""ilu0_csr (include/spmv/ilu0.h) on the GPU: the device factor against ilu0_cpu_csr at zero tolerance for every lane
count, out of place and in place, over shapes that reach both launch kinds, the 8192-level split, rows longer than
64 * 4 entries and rows of one entry; the schedule cache; the async entry on a side stream; rejection before
d_lu_values is written; the reported zero pivot; and the factor put to use by two sptrsv_csr calls."""
import ctypes
import importlib

import numpy as np
import pytest

import ilu0_cases as cases
import test_gpu_sptrsv as trsv
from test_gpu_sptrsv import _assert_same_bits, _bits

pytestmark = pytest.mark.gpu

LANES = (1, 2, 4, 8, 16, 32, 64)
NARROW = 256          # csrc/internal.h kSptrsvNarrowRows
MAX_RUN = 8192        # csrc/internal.h kSptrsvMaxRunLevels

nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
spd = importlib.import_module("gpu-spmv_amd.spd")


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


def _factor(gpu, A, va, in_place, sentinel=None):
    """(result, lu values); in place factors A's own device values and puts A's values back afterwards"""
    nnz = int(A.contents.nnz)
    if in_place:
        res = gpu.ilu0_csr(A, A.contents.d_values)
        lu = _download(gpu, A.contents.d_values, nnz)
        _restore(gpu, A, va)
        return res, lu
    d_lu = gpu.CudaBuffer(max(nnz, 1))
    d_lu.copyFromHost(np.full(max(nnz, 1), np.nan if sentinel is None else sentinel, np.float32), max(nnz, 1))
    res = gpu.ilu0_csr(A, d_lu)
    lu = d_lu.copyToHost(max(nnz, 1))[:nnz]
    d_lu.release()
    return res, lu


def _dense_csr(dense):
    dense = np.asarray(dense, np.float32)
    rows, cols = np.nonzero(dense)
    return cases.csr_from_coo(dense.shape[0], rows, cols, dense[rows, cols])


SHAPES = {
    "n=1": lambda: _dense_csr([[5.0]]),
    "n=2": lambda: _dense_csr([[4.0, 1.0], [2.0, 3.0]]),
    "tridiagonal(257)": lambda: cases.exact_tridiagonal(257)[:4],
    "tridiagonal(8193+64)": lambda: cases.exact_tridiagonal(MAX_RUN + 1 + 64)[:4],
    "convdiff2d(24,(3,.5))": lambda: nonsym.convdiff2d(24, (3.0, 0.5)),
    "convdiff3d(24)": lambda: nonsym.convdiff3d(24, 1.0),
    "600 dense 3x3 blocks": lambda: cases.block3(600),
    "arrow(300)": lambda: cases.arrow(300),
    "sorted_random(2000,7)": lambda: cases.sorted_random(2000, 7, 11),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_factor_equals_the_cpu_bit_for_bit_at_every_lane_count(gpu, monkeypatch, name):
    n, rp, ci, va = SHAPES[name]()
    A = _upload(gpu, n, rp, ci, va)
    want, want_pivot = gpu.ilu0_cpu_csr(A)
    assert want_pivot == -1
    _, level_ptr, _, levels, _ = gpu.sptrsv_levels(n, rp, ci, 0)
    widths = np.diff(level_ptr)
    launches = None
    # what the shape is here for
    if name.startswith("tridiagonal"):
        fact = cases.exact_tridiagonal(n)[4]
        np.testing.assert_array_equal(_bits(cases.prove_exact(n, rp, ci, va)), _bits(fact))
        np.testing.assert_array_equal(_bits(want), _bits(fact))
        assert levels == n
        launches = 2 if n > MAX_RUN else 1
    elif name.startswith("arrow"):
        np.testing.assert_array_equal(_bits(want), _bits(cases.prove_exact(n, rp, ci, va, shift=3)))
        assert np.diff(rp).max() == n > 64 * 4 and np.bincount(ci).max() == n
    elif name.startswith("convdiff2d"):
        assert widths.max() <= NARROW and levels > 1
        launches = 1
    elif name.startswith("convdiff3d"):
        assert (widths > NARROW).any() and (widths <= NARROW).any()
    elif name.startswith("600"):
        assert widths.tolist() == [600, 600, 600]
        launches = 3
    try:
        for lanes in LANES + (None,):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"ilu0_lanes={lanes}")
            for in_place in (False, True):
                res, got = _factor(gpu, A, va, in_place)
                tag = f"{name} lanes={lanes} in_place={in_place}"
                assert res.error_code == 0 and res.zero_pivot == -1 and res.num_levels == levels, tag
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
    """SPMV_DEBUG=ilu0_lanes=v with v outside 1, 2, 4, ... 64 changes nothing: the library's own pick, the CPU's bits."""
    n, rp, ci, va = spd.poisson2d(8)
    assert n == 64
    A = _upload(gpu, n, rp, ci, va)
    want, _ = gpu.ilu0_cpu_csr(A)
    try:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        own, got = _factor(gpu, A, va, False)
        assert own.error_code == 0 and own.lanes_per_row in LANES
        np.testing.assert_array_equal(_bits(got), _bits(want))
        for value in (0, 3, 128, -4):
            monkeypatch.setenv("SPMV_DEBUG", f"ilu0_lanes={value}")
            res, got = _factor(gpu, A, va, False)
            assert res.error_code == 0 and res.lanes_per_row == own.lanes_per_row, value
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(value))
        for lanes in (1, 64):                    # the ends of the range are taken
            monkeypatch.setenv("SPMV_DEBUG", f"ilu0_lanes={lanes}")
            res, got = _factor(gpu, A, va, False)
            assert res.error_code == 0 and res.lanes_per_row == lanes
            np.testing.assert_array_equal(_bits(got), _bits(want))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


def test_schedule_cache_and_the_async_entry(gpu):
    import torch
    n, rp, ci, va = nonsym.convdiff3d(12, 1.0)
    A = _upload(gpu, n, rp, ci, va)
    want, _ = gpu.ilu0_cpu_csr(A)
    first, lu0 = _factor(gpu, A, va, False)
    assert first.error_code == 0 and first.analysis_ms > 0 and first.elapsed_ms > 0
    second, lu1 = _factor(gpu, A, va, False)
    assert second.analysis_ms == 0
    assert (second.num_levels, second.launches, second.lanes_per_row) == (first.num_levels, first.launches,
                                                                         first.lanes_per_row)
    np.testing.assert_array_equal(_bits(lu0), _bits(want))
    np.testing.assert_array_equal(_bits(lu1), _bits(want))
    # the schedule is sptrsv_csr's LOWER one: already there for a solve, and the other way round
    assert gpu.sptrsv_analyze(A, 0).analysis_ms == 0
    gpu.csr_invalidate_gpu_cache(A)
    again, lu2 = _factor(gpu, A, va, False)
    assert again.analysis_ms > 0 and _factor(gpu, A, va, False)[0].analysis_ms == 0
    np.testing.assert_array_equal(_bits(lu2), _bits(want))
    gpu.csr_invalidate_gpu_cache(A)
    assert gpu.sptrsv_analyze(A, 0).analysis_ms > 0 and _factor(gpu, A, va, False)[0].analysis_ms == 0
    # a side stream, out of place and in place
    stream = torch.cuda.Stream()
    out = torch.full((ci.size,), float("nan"), device="cuda")
    own = torch.from_numpy(va).cuda()
    W = gpu.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, own.data_ptr())
    torch.cuda.synchronize()
    assert gpu.ilu0_csr_async(A, out.data_ptr(), stream.cuda_stream) == 0
    assert gpu.ilu0_csr_async(W, own.data_ptr(), stream.cuda_stream) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(own.cpu().numpy()), _bits(want))
    gpu.csr_destroy(W)
    gpu.csr_destroy(A)


def test_rejections_leave_the_output_untouched(gpu):
    E = gpu.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    n, rp, ci, va = nonsym.random_nonsym(500, 7, 1)                    # as generated: repeated columns, diagonal last
    bad = {
        "unsorted row": (3, [0, 2, 4, 6], [0, 1, 1, 0, 1, 2], f32([4, 1, 4, 1, 1, 4]), E.INVALID_ARGUMENT),
        "repeated column": (3, [0, 2, 5, 6], [0, 1, 0, 1, 1, 2], f32([4, 1, 1, 2, 2, 4]), E.INVALID_ARGUMENT),
        "missing diagonal": (3, [0, 2, 3, 5], [0, 1, 0, 1, 2], f32([4, 1, 1, 1, 4]), E.INVALID_ARGUMENT),
        "random_nonsym": (n, rp, ci, va, E.INVALID_ARGUMENT),
        "column out of range": (3, [0, 2, 4, 6], [0, 1, 0, 1, 1, 7], f32([4, 1, 1, 4, 1, 4]), E.INVALID_FORMAT),
        "row_ptrs decrease": (3, [0, 4, 2, 6], [0, 1, 0, 1, 1, 2], f32([4, 1, 1, 4, 1, 4]), E.INVALID_FORMAT),
    }
    for name, (rows, ptr, col, val, code) in bad.items():
        A = _upload(gpu, rows, ptr, col, val)
        res, lu = _factor(gpu, A, val, False, sentinel=-77.0)
        assert res.error_code == code and (lu == -77.0).all(), name
        assert gpu.ilu0_csr(A, A.contents.d_values).error_code == code, name            # in place: A's values stay
        np.testing.assert_array_equal(_bits(_download(gpu, A.contents.d_values, len(val))), _bits(val), err_msg=name)
        d_lu = gpu.CudaBuffer(len(val))
        d_lu.copyFromHost(np.full(len(val), -77.0, np.float32), len(val))
        assert gpu.ilu0_csr_async(A, d_lu, None) == code, name
        assert (d_lu.copyToHost(len(val)) == -77.0).all(), name
        d_lu.release()
        gpu.csr_destroy(A)
    # a partial overlap with A's device values
    n, rp, ci, va = nonsym.convdiff2d(8, 1.0)
    A = _upload(gpu, n, rp, ci, va)
    assert gpu.ilu0_csr(A, A.contents.d_values + 4).error_code == E.INVALID_ARGUMENT
    np.testing.assert_array_equal(_bits(_download(gpu, A.contents.d_values, ci.size)), _bits(va))
    gpu.csr_destroy(A)


def test_zero_pivot_is_reported_like_the_cpu(gpu, monkeypatch):
    dense_cases = {
        "zero a_00": ([[0, 1, 0], [1, 4, 1], [0, 1, 4]], 0),
        "cancels at row 2": ([[2, 0, 0, 0], [0, 1, 3, 0], [0, 2, 6, 1], [0, 0, 1, 4]], 2),
        "clean": ([[4, 1, 0], [1, 4, 1], [0, 1, 4]], -1),
    }
    for name, (dense, want_pivot) in dense_cases.items():
        dense = np.asarray(dense, np.float32)
        n = dense.shape[0]
        rows, cols = np.nonzero(dense)
        keep = dense[rows, cols]
        if name == "zero a_00":                                  # the zero is a STORED entry
            rows, cols, keep = np.r_[0, rows], np.r_[0, cols], np.r_[np.float32(0), keep]
        _, rp, ci, va = cases.csr_from_coo(n, rows, cols, keep)
        A = _upload(gpu, n, rp, ci, va)
        want, cpu_pivot = gpu.ilu0_cpu_csr(A)
        assert cpu_pivot == want_pivot, name
        for lanes in (1, 4, None):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"ilu0_lanes={lanes}")
            for in_place in (False, True):
                res, got = _factor(gpu, A, va, in_place)
                assert (res.error_code, res.zero_pivot) == (0, want_pivot), (name, lanes, in_place)
                _assert_same_bits(got, want, name)
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
    # a pivot far down a larger matrix: the lowest bad row wins whatever the order the scan meets them in
    n, rp, ci, va = nonsym.convdiff3d(12, 1.0)
    va = va.copy()
    r = cases.rows_of(n, rp)
    for row in (1500, 900, 1300):
        va[(r == row)] = 0.0
        va[(ci == row) & (r != row)] = 0.0                        # nothing updates (row, row): it stays exactly 0
    A = _upload(gpu, n, rp, ci, va)
    want, cpu_pivot = gpu.ilu0_cpu_csr(A)
    res, got = _factor(gpu, A, va, False)
    assert cpu_pivot == 900 and (res.error_code, res.zero_pivot) == (0, 900)
    _assert_same_bits(got, want)
    gpu.csr_destroy(A)


def test_the_factor_solves_through_two_triangular_solves(gpu):
    rng = np.random.default_rng(12)
    lower, upper = gpu.SpTRSVConfig(uplo=0, diag=1), gpu.SpTRSVConfig(uplo=1, diag=0)
    systems = {"tridiagonal(257)": cases.exact_tridiagonal(257)[:4], "convdiff2d(24)": nonsym.convdiff2d(24, (3.0, .5)),
               "sorted_random(2000,7)": cases.sorted_random(2000, 7, 11)}
    for name, (n, rp, ci, va) in systems.items():
        A = _upload(gpu, n, rp, ci, va)
        d_lu = gpu.CudaBuffer(ci.size)
        assert gpu.ilu0_csr(A, d_lu).error_code == 0
        lu = d_lu.copyToHost(ci.size)
        F = gpu.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, d_lu.get())
        exact = name.startswith("tridiagonal")
        if exact:                              # A = L U exactly: x of small integers, b = A x exact in fp32
            x_true = rng.integers(-3, 4, n).astype(np.float32)
            b = importlib.import_module("gpu-spmv_amd.spd").spmv64(rp, ci, va, x_true).astype(np.float32)
        else:
            b = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        d_b, d_y = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        d_b.copyFromHost(b, n)
        first = gpu.sptrsv_csr(F, d_b, d_y, lower)
        assert first.error_code == 0 and first.analysis_ms == 0      # the factor shares A's LOWER schedule
        y = d_y.copyToHost(n)
        assert gpu.sptrsv_csr(F, d_y, d_y, upper).error_code == 0
        x = d_y.copyToHost(n)
        if exact:
            np.testing.assert_array_equal(_bits(x), _bits(x_true))
        else:
            assert np.isfinite(x).all()
            assert trsv.backward_error_ratio(n, rp, ci, lu, b, y, 0, 1) <= 1.0, name
            assert trsv.backward_error_ratio(n, rp, ci, lu, y, x, 1, 0) <= 1.0, name
        for buf in (d_b, d_y, d_lu):
            buf.release()
        gpu.csr_destroy(F)
        gpu.csr_destroy(A)
