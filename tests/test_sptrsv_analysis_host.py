"""The device-side level analysis (include/spmv/sptrsv.h sptrsv_analyze_device, sptrsv_schedule_get; DESIGN.md
§4.23) on the host side (no GPU): the exported names and the info struct's layout; the argument checks of both entry
points in their documented order, on fake device addresses they must return before touching; and the numpy
restatement of the device's one_sided_row rule, whose SIGN is held against detail::one_sided_row through
ic0_cpu_csr's accept / reject."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import sptrsv_analysis_cases as cases
from conftest import ROOT

NAMES = ("sptrsv_analyze_device", "sptrsv_schedule_get")

# fake, never-dereferenced device addresses: every call below must return before it touches them
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


def test_names_in_both_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    cxx = open(os.path.join(ROOT, "include", "spmv", "sptrsv.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared, name
        assert "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name), name
        assert callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert "spmv_c_sptrsv_schedule_info" in header and re.search(r"\bstruct SpTRSVScheduleInfo\b", cxx)


def test_info_struct_size_and_offsets(spmv):
    info = spmv.SpTRSVScheduleInfo
    fields = ["num_levels", "launches", "first_missing_diagonal", "first_unsorted_row", "one_sided_row",
              "built_on_device", "triangle_nnz"]
    assert ctypes.sizeof(info) == 32
    assert [f for f, _ in info._fields_] == fields
    assert [getattr(info, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24]
    assert [getattr(info, f).size for f in fields] == [4, 4, 4, 4, 4, 4, 8]
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    body = re.search(r"typedef struct spmv_c_sptrsv_schedule_info \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"int(?:32|64)_t\s+(\w+);", body) == fields
    assert re.findall(r"(int(?:32|64)_t)\s+\w+;", body) == ["int32_t"] * 6 + ["int64_t"]


def _host_matrix(spmv, rows=8, cols=8):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, i % cols] = 4.0
        dense[i, (i + 1) % cols] = -1.0
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


def test_analyze_device_checks_in_sptrsv_analyzes_order(spmv):
    E = spmv.SpMVError
    for analyze in (spmv.sptrsv_analyze_device, spmv.sptrsv_analyze):          # the same checks, the same order
        assert analyze(None, 0).error_code == E.INVALID_ARGUMENT
        R = spmv.csr_create(5, 4, 0)
        assert analyze(R, 9).error_code == E.INVALID_DIMENSION               # not square, before uplo
        spmv.csr_destroy(R)
        Z = spmv.csr_create(0, 0, 0)
        res = analyze(Z, 9)
        assert (res.error_code, res.num_levels, res.launches, res.analysis_ms) == (E.SUCCESS, 0, 0, 0.0)
        spmv.csr_destroy(Z)
        A = _host_matrix(spmv)
        assert analyze(A, 9).error_code == E.INVALID_FORMAT                  # host-only, before uplo
        spmv.csr_destroy(A)
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
        assert analyze(D, 0).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(D)
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
        for uplo in (2, -1, 7):
            assert analyze(D, uplo).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
    A = _host_matrix(spmv)
    out = spmv.SpTRSVResult(error_code=7, num_levels=9)
    assert spmv.lib().spmv_c_sptrsv_analyze_device(A, 0, ctypes.byref(out)) == E.INVALID_FORMAT
    assert out.error_code == E.INVALID_FORMAT and out.num_levels == 0
    assert spmv.lib().spmv_c_sptrsv_analyze_device(A, 0, None) == E.INVALID_FORMAT   # out may be NULL
    spmv.csr_destroy(A)


def test_schedule_get_checks_and_writes_nothing_without_a_schedule(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    level_ptr = np.full(9, -5, np.int32)
    order = np.full(8, -5, np.int32)
    info = spmv.SpTRSVScheduleInfo(-5, -5, -5, -5, -5, -5, -5)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def untouched():
        return ((level_ptr == -5).all() and (order == -5).all() and
                [getattr(info, f) for f, _ in info._fields_] == [-5] * 7)

    # 1. null A, before uplo
    assert lib.spmv_c_sptrsv_schedule_get(None, 9, ptr(level_ptr), ptr(order), ctypes.byref(info)) == E.INVALID_ARGUMENT
    # 2. uplo, before the cache is asked
    D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    for uplo in (2, -1):
        assert lib.spmv_c_sptrsv_schedule_get(D, uplo, ptr(level_ptr), ptr(order), ctypes.byref(info)) == E.INVALID_ARGUMENT
    # 3. no schedule: a device matrix never analysed, a host-only matrix, an empty one
    A = _host_matrix(spmv)
    Z = spmv.csr_create(0, 0, 0)
    for M in (D, A, Z):
        for uplo in (0, 1):
            assert lib.spmv_c_sptrsv_schedule_get(M, uplo, ptr(level_ptr), ptr(order), ctypes.byref(info)) == E.INVALID_ARGUMENT
            assert lib.spmv_c_sptrsv_schedule_get(M, uplo, None, None, None) == E.INVALID_ARGUMENT
            assert spmv.sptrsv_schedule_get(M, uplo) == (E.INVALID_ARGUMENT, None, None, None)
            assert spmv.sptrsv_schedule_get(M, uplo, arrays=False) == (E.INVALID_ARGUMENT, None, None, None)
    assert spmv.sptrsv_schedule_get(None, 0)[0] == E.INVALID_ARGUMENT
    assert untouched()
    for M in (D, A, Z):
        spmv.csr_destroy(M)


def test_device_one_sided_rule_agrees_in_sign_with_the_host_pass(spmv, spd):
    """ic0_cpu_csr rejects a sorted pattern with every diagonal exactly when detail::one_sided_row names a row"""
    saw = set()
    for name, ((n, rp, ci, va), symmetric) in cases.one_sided_variants(spd).items():
        assert cases.first_unsorted_row(n, rp, ci) == -1, name
        want = cases.one_sided_row(n, rp, ci)
        assert (want < 0) == symmetric, (name, want)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        try:
            spmv.ic0_cpu_csr(A)
            accepted = True
        except ValueError:
            accepted = False
        spmv.csr_destroy(A)
        assert accepted == (want < 0), (name, want)
        saw.add(accepted)
    assert saw == {True, False}
    # the GPU file's own families, where the rows are sorted and every diagonal is stored (the LOWER schedules whose
    # one_sided_row is tested at all)
    nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
    tested = {}
    for name, (n, rp, ci, va) in cases.families(spd, nonsym).items():
        if cases.first_unsorted_row(n, rp, ci) >= 0 or spmv.sptrsv_levels(n, rp, ci, 0)[4] >= 0:
            continue
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        try:
            spmv.ic0_cpu_csr(A)
            accepted = True
        except ValueError:
            accepted = False
        spmv.csr_destroy(A)
        tested[name] = cases.one_sided_row(n, rp, ci)
        assert accepted == (tested[name] < 0), (name, tested[name])
    assert {"n=1", "n=2", "diagonal(257)", "chain(300)", "staircase", "poisson3d(32)", "arrow(5000)"} <= set(tested)
    assert tested["arrow(5000)"] == 1 and tested["staircase"] == 255 and tested["poisson3d(32)"] == -1
    # the value: the LOWEST row with a stored (i,k) whose (k,i) is missing
    n, rp, ci, _ = cases.one_sided_variants(spd)["poisson2d(12) less (40,41)"][0]
    assert cases.one_sided_row(n, rp, ci) == 41
    n, rp, ci, _ = cases.one_sided_variants(spd)["poisson2d(12) less (77,76)"][0]
    assert cases.one_sided_row(n, rp, ci) == 76
    assert cases.one_sided_row(*cases.arrow(50)[:3]) == 1                      # (1, 0) without (0, 1)
    assert cases.one_sided_row(*cases.staircase([3, 4, 5, 1, 6])[:3]) == 3


def test_case_generators_have_the_shapes_the_gpu_file_relies_on(spmv, spd):
    widths = [255, 256, 257, 1, 600, 256]
    n, rp, ci, _ = cases.staircase(widths)
    status, level_ptr, order, levels, missing = spmv.sptrsv_levels(n, rp, ci, 0)
    assert status == 0 and np.diff(level_ptr).tolist() == widths and missing == -1
    assert cases.launches(level_ptr) == 5                        # 255+256 | 257 | 1 | 600 | 256
    status, level_ptr, _, levels, _ = spmv.sptrsv_levels(*cases.flipped((n, rp, ci, None))[:3], 1)
    assert status == 0 and np.diff(level_ptr).tolist() == widths
    n, rp, ci, _ = cases.chain(cases.MAX_RUN_LEVELS + 5)
    for uplo in (0, 1):
        status, level_ptr, _, levels, _ = spmv.sptrsv_levels(n, rp, ci, uplo)
        assert levels == n and cases.launches(level_ptr) == 2
    n, rp, ci, _ = cases.arrow(5000)
    assert int(np.diff(rp).max()) == n and int(np.bincount(ci).max()) == n
    assert spmv.sptrsv_levels(n, rp, ci, 0)[3] == 3 and spmv.sptrsv_levels(n, rp, ci, 1)[3] == 1
    n, rp, ci, _ = cases.strictly_lower(700)
    assert spmv.sptrsv_levels(n, rp, ci, 1)[3] == 1 and spmv.sptrsv_levels(n, rp, ci, 0)[3] > 3
    assert spmv.sptrsv_levels(n, rp, ci, 0)[4] == 0
    nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
    n, rp, ci, _ = cases.messy(nonsym)
    r = np.repeat(np.arange(n), np.diff(rp))
    assert cases.first_unsorted_row(n, rp, ci) >= 0 and spmv.sptrsv_levels(n, rp, ci, 0)[4] >= 0
    assert (np.diff(rp) == 0).any() and np.unique(r * n + ci.astype(np.int64)).size < ci.size
