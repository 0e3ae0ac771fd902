"""ilu0_csr / ilu0_cpu_csr / bicgstab_solve_lu (include/spmv/ilu0.h, include/spmv/bicgstab.h) on the host side (no
GPU): the exported names and the ILU0Result layout; ilu0_cpu_csr against a numpy restatement of the documented
arithmetic, bit for bit; integer matrices whose exact LU is proven in int64 first (tests/ilu0_cases.py) and must come
back exactly; the rejections in their documented order through the C ABI and Python with the output untouched; the
reported zero pivot."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import ilu0_cases as cases
from conftest import ROOT

NAMES = ("ilu0_csr", "ilu0_csr_async", "ilu0_cpu_csr")

# fake, never-dereferenced device addresses: every call below must return before it touches them
LU, B, X = 0x100000, 0x600000, 0x700000
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


@pytest.fixture(scope="module")
def nonsym():
    return importlib.import_module("gpu-spmv_amd.nonsym")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- names and layouts ---------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)                     # what test_host_library.py checks
    cxx = open(os.path.join(ROOT, "include", "spmv", "ilu0.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared and "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert "spmv_c_bicgstab_solve_lu" in declared and "spmv_c_bicgstab_solve_lu" in spmv.EXPORTED_SYMBOLS
    assert hasattr(spmv.lib(), "spmv_c_bicgstab_solve_lu") and callable(spmv.bicgstab_solve_lu)
    assert re.search(r"\bbicgstab_solve_lu\s*\(", open(os.path.join(ROOT, "include", "spmv", "bicgstab.h")).read())


def test_result_layout(spmv):
    assert ctypes.sizeof(spmv.ILU0Result) == 28
    names = ["error_code", "num_levels", "launches", "lanes_per_row", "zero_pivot", "analysis_ms", "elapsed_ms"]
    assert [f for f, _ in spmv.ILU0Result._fields_] == names
    assert [getattr(spmv.ILU0Result, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24]


# ---- the arithmetic ------------------------------------------------------------------------------------------
def test_cpu_factorisation_equals_the_numpy_restatement_bit_for_bit(spmv, nonsym):
    for name, (n, rp, ci, va) in (("convdiff2d(8)", nonsym.convdiff2d(8, 1.0)),
                                  ("sorted_random(40,5)", cases.sorted_random(40, 5, 3))):
        assert (np.diff(ci)[np.diff(cases.rows_of(n, rp)) == 0] > 0).all()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        got, pivot = spmv.ilu0_cpu_csr(A)
        want, want_pivot = cases.numpy_ilu0(n, rp, ci, va)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=name)
        assert pivot == want_pivot == -1
        assert not np.array_equal(_bits(got), _bits(va))                # it did factor something
        # in place through the C ABI: lu_values is A's own host array
        inplace = va.copy()
        H = spmv.csr_from_arrays(n, n, rp, ci, inplace)
        host_values = ctypes.cast(H.contents.values, ctypes.c_void_p)
        assert spmv.lib().spmv_c_ilu0_cpu_csr(H, host_values, None) == 0
        np.testing.assert_array_equal(_bits(np.ctypeslib.as_array(H.contents.values, shape=(ci.size,))), _bits(want))
        spmv.csr_destroy(H)
        spmv.csr_destroy(A)


def test_exact_integer_factors_come_back_exactly(spmv):
    tri = [cases.exact_tridiagonal(50), cases.exact_tridiagonal(64, seed=2)]
    for n, rp, ci, va, fact in tri:
        proven = cases.prove_exact(n, rp, ci, va)
        np.testing.assert_array_equal(_bits(proven), _bits(fact))       # the bidiagonals it was built from
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        got, pivot = spmv.ilu0_cpu_csr(A)
        np.testing.assert_array_equal(_bits(got), _bits(fact))
        assert pivot == -1
        spmv.csr_destroy(A)
    n, rp, ci, va = cases.arrow(40)
    proven = cases.prove_exact(n, rp, ci, va, shift=3)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    got, pivot = spmv.ilu0_cpu_csr(A)
    np.testing.assert_array_equal(_bits(got), _bits(proven))
    assert pivot == -1 and not np.array_equal(got[rp[n - 1]:], va[rp[n - 1]:])
    spmv.csr_destroy(A)


# ---- rejections ----------------------------------------------------------------------------------------------
def _cpu_rejects(spmv, n, cols, rp, ci, va, code):
    A = spmv.csr_from_arrays(n, cols, rp, ci, va)
    out = np.full(max(len(va), 1), -77.0, np.float32)
    pivot = ctypes.c_int32(55)
    status = spmv.lib().spmv_c_ilu0_cpu_csr(A, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pivot))
    assert status == code and (out == -77.0).all()
    with pytest.raises(ValueError):
        spmv.ilu0_cpu_csr(A)
    spmv.csr_destroy(A)


def test_cpu_rejections_leave_the_output_untouched(spmv, nonsym):
    E = spmv.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    # unsorted row; repeated column; missing diagonal; not square
    _cpu_rejects(spmv, 3, 3, [0, 2, 4, 6], [0, 1, 1, 0, 1, 2], f32([4, 1, 4, 1, 1, 4]), E.INVALID_ARGUMENT)
    _cpu_rejects(spmv, 3, 3, [0, 2, 5, 6], [0, 1, 0, 1, 1, 2], f32([4, 1, 1, 2, 2, 4]), E.INVALID_ARGUMENT)
    _cpu_rejects(spmv, 3, 3, [0, 2, 3, 5], [0, 1, 0, 1, 2], f32([4, 1, 1, 1, 4]), E.INVALID_ARGUMENT)
    _cpu_rejects(spmv, 2, 3, [0, 1, 2], [0, 1], f32([4, 4]), E.INVALID_DIMENSION)
    n, rp, ci, va = nonsym.random_nonsym(200, 7, 1)                     # as generated: diagonal last, columns repeat
    _cpu_rejects(spmv, n, n, rp, ci, va, E.INVALID_ARGUMENT)
    # malformed arrays come before the sorting rule
    _cpu_rejects(spmv, 3, 3, [0, 2, 4, 6], [0, 1, 1, 0, 1, 7], f32([4, 1, 4, 1, 1, 4]), E.INVALID_FORMAT)
    # nulls
    lib = spmv.lib()
    A = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], f32([4, 4]))
    out = np.zeros(2, np.float32)
    assert lib.spmv_c_ilu0_cpu_csr(None, out.ctypes.data_as(ctypes.c_void_p), None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_ilu0_cpu_csr(A, None, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_ilu0_cpu_csr(A, out.ctypes.data_as(ctypes.c_void_p), None) == 0      # zero_pivot may be NULL
    spmv.csr_destroy(A)
    Z = spmv.csr_create(0, 0, 0)
    pivot = ctypes.c_int32(9)
    assert lib.spmv_c_ilu0_cpu_csr(Z, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pivot)) == 0
    assert pivot.value == -1
    spmv.csr_destroy(Z)


def _c_call(spmv, A, lu):
    out = spmv.ILU0Result(error_code=12345, zero_pivot=99)
    rc = spmv.lib().spmv_c_ilu0_csr(A, ctypes.c_void_p(lu), ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_device_entry_checks_in_the_stated_order_before_any_device_work(spmv):
    E = spmv.SpMVError
    for call in (lambda A, lu: _c_call(spmv, A, lu), lambda A, lu: spmv.ilu0_csr(A, lu),
                 lambda A, lu: spmv.ILU0Result(error_code=spmv.lib().spmv_c_ilu0_csr_async(A, ctypes.c_void_p(lu),
                                                                                          None))):
        # 1. nulls
        assert call(None, LU).error_code == E.INVALID_ARGUMENT
        R = spmv.csr_create(5, 4, 0)
        assert call(R, None).error_code == E.INVALID_ARGUMENT
        # 2. not square, before the empty and format checks
        assert call(R, LU).error_code == E.INVALID_DIMENSION
        spmv.csr_destroy(R)
        # 3. no rows: SUCCESS
        Z = spmv.csr_create(0, 0, 0)
        res = call(Z, LU)
        assert (res.error_code, res.num_levels, res.launches) == (E.SUCCESS, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (a host-only matrix; a wrap without columns)
        H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], np.asarray([4, 4], np.float32))
        assert call(H, LU).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(H)
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
        assert call(D, FAKE_VA + 4).error_code == E.INVALID_FORMAT       # before the overlap check
        spmv.csr_destroy(D)
        # 5. partial overlap with A's values (16 floats = 64 bytes); the same array is checked later, not here
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
        for lu in (FAKE_VA + 4, FAKE_VA + 60, FAKE_VA - 60, FAKE_VA - 4):
            assert call(D, lu).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
    out = spmv.ILU0Result(error_code=7, num_levels=9)
    assert spmv.lib().spmv_c_ilu0_csr(None, ctypes.c_void_p(LU), ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and out.num_levels == 0 and out.zero_pivot == -1
    assert spmv.lib().spmv_c_ilu0_csr(None, ctypes.c_void_p(LU), None) == E.INVALID_ARGUMENT      # out may be NULL


def test_bicgstab_solve_lu_checks_before_any_device_work(spmv):
    E = spmv.SpMVError
    D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    F = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, LU)
    code = lambda *a: spmv.bicgstab_solve_lu(*a).error_code
    # nulls first, the factor among them
    assert code(None, F, B, X) == E.INVALID_ARGUMENT
    assert code(D, None, B, X) == E.INVALID_ARGUMENT
    assert code(D, F, None, X) == E.INVALID_ARGUMENT
    assert code(D, F, B, None) == E.INVALID_ARGUMENT
    # dimensions: A's, then the factor's (not square; another size), before the empty system and the formats
    R = spmv.csr_create(5, 4, 0)
    S9 = spmv.csr_wrap_device(9, 9, 16, FAKE_RP, FAKE_CI, LU)
    Z = spmv.csr_create(0, 0, 0)
    assert code(R, F, B, X) == E.INVALID_DIMENSION
    assert code(D, R, B, X) == E.INVALID_DIMENSION
    assert code(D, S9, B, X) == E.INVALID_DIMENSION
    assert code(Z, F, B, X) == E.INVALID_DIMENSION
    res = spmv.bicgstab_solve_lu(Z, Z, B, X)
    assert (res.error_code, res.converged, res.iterations) == (0, 1, 0)
    # device arrays of either matrix
    H = spmv.csr_from_arrays(8, 8, np.arange(9, dtype=np.int32), np.arange(8, dtype=np.int32), np.ones(8, np.float32))
    bad_cfg = spmv.BiCGStabConfig(tolerance=-1.0)
    assert code(H, F, B, X, bad_cfg) == E.INVALID_FORMAT
    assert code(D, H, B, X, bad_cfg) == E.INVALID_FORMAT
    # the config (its preconditioner is not read), then the overlap of b and x
    assert code(D, F, B, B + 4, bad_cfg) == E.INVALID_ARGUMENT
    assert code(D, F, B, X, spmv.BiCGStabConfig(max_iterations=-1)) == E.INVALID_ARGUMENT
    assert code(D, F, B, X, spmv.BiCGStabConfig(engine=2)) == E.INVALID_ARGUMENT
    assert code(D, F, B, B + 4, spmv.BiCGStabConfig(preconditioner=2)) == E.INVALID_ARGUMENT        # the overlap
    assert code(D, F, B, B) == E.INVALID_ARGUMENT
    # bicgstab_solve itself still rejects an unknown preconditioner
    assert spmv.bicgstab_solve(D, B, X, spmv.BiCGStabConfig(preconditioner=2)).error_code == E.INVALID_ARGUMENT
    out = spmv.BiCGStabResult(error_code=7, iterations=9)
    assert spmv.lib().spmv_c_bicgstab_solve_lu(D, None, ctypes.c_void_p(B), ctypes.c_void_p(X), None,
                                               ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and out.iterations == 0
    assert spmv.lib().spmv_c_bicgstab_solve_lu(D, None, ctypes.c_void_p(B), ctypes.c_void_p(X), None,
                                               None) == E.INVALID_ARGUMENT
    for M in (D, F, R, S9, Z, H):
        spmv.csr_destroy(M)


# ---- pivots --------------------------------------------------------------------------------------------------
def test_zero_pivot_is_reported_and_is_not_an_error(spmv):
    f32 = lambda v: np.asarray(v, np.float32)
    dense_cases = {
        "zero a_00": ([[0, 1, 0], [1, 4, 1], [0, 1, 4]], 0),
        # row 2: l_21 = 2 / 1, u_22 = 6 - 2 * 3 = 0
        "cancels at row 2": ([[2, 0, 0, 0], [0, 1, 3, 0], [0, 2, 6, 1], [0, 0, 1, 4]], 2),
        "clean": ([[4, 1, 0], [1, 4, 1], [0, 1, 4]], -1),
    }
    for name, (dense, want) in dense_cases.items():
        dense = f32(dense)
        n = dense.shape[0]
        rows, cols = np.nonzero(dense)
        keep = dense[rows, cols]
        if name == "zero a_00":                                  # the zero is a STORED entry
            rows, cols, keep = np.r_[0, rows], np.r_[0, cols], np.r_[np.float32(0), keep]
        _, rp, ci, va = cases.csr_from_coo(n, rows, cols, keep)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        with np.errstate(all="ignore"):
            got, pivot = spmv.ilu0_cpu_csr(A)
            ref, ref_pivot = cases.numpy_ilu0(n, rp, ci, va)
        assert pivot == ref_pivot == want, name
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name)
        np.testing.assert_array_equal(_bits(got)[~np.isnan(ref)], _bits(ref)[~np.isnan(ref)], err_msg=name)
        spmv.csr_destroy(A)
