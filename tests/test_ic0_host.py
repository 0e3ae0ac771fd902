"""ic0_csr / ic0_cpu_csr / cg_solve_ic (include/spmv/ic0.h, include/spmv/cg.h) on the host side (no GPU): the exported
names and the IC0Result layout; ic0_cpu_csr against a numpy restatement of the documented arithmetic, bit for bit;
dyadic matrices whose exact Cholesky factor is proven in integers first (tests/ic0_cases.py) and must come back
exactly; L^T in the upper positions; in place against out of place; the reported bad pivot; the rejections through the
C ABI and Python with the output untouched; the checks of the device entries that come before any device work; and
the sanitized caller of ic0_cpu_csr."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import ic0_cases as cases
from conftest import ROOT

NAMES = ("ic0_csr", "ic0_csr_async", "ic0_cpu_csr")

# fake, never-dereferenced device addresses: every call below must return before it touches them
L, B, X = 0x100000, 0x600000, 0x700000
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- names and layouts ---------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)                     # what test_host_library.py checks
    cxx = open(os.path.join(ROOT, "include", "spmv", "ic0.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared and "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert "spmv_c_cg_solve_ic" in declared and "spmv_c_cg_solve_ic" in spmv.EXPORTED_SYMBOLS
    assert hasattr(spmv.lib(), "spmv_c_cg_solve_ic") and callable(spmv.cg_solve_ic)
    assert re.search(r"\bcg_solve_ic\s*\(", open(os.path.join(ROOT, "include", "spmv", "cg.h")).read())


def test_result_layout(spmv):
    assert ctypes.sizeof(spmv.IC0Result) == 28
    names = ["error_code", "num_levels", "launches", "lanes_per_row", "bad_pivot", "analysis_ms", "elapsed_ms"]
    assert [f for f, _ in spmv.IC0Result._fields_] == names
    assert [getattr(spmv.IC0Result, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24]


# ---- the arithmetic ------------------------------------------------------------------------------------------
def test_cpu_factorisation_equals_the_numpy_restatement_bit_for_bit(spmv, spd):
    for name, (n, rp, ci, va) in (("poisson2d(12)", spd.poisson2d(12)),
                                  ("sorted_random_spd(200,8)", cases.sorted_random_spd(200, 8, 3)),
                                  ("spd_blocks(40)", cases.spd_blocks(40)),
                                  ("arrow_spd(70)", cases.arrow_spd(70))):
        assert (np.diff(ci)[np.diff(cases.rows_of(n, rp)) == 0] > 0).all()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        got, pivot = spmv.ic0_cpu_csr(A)
        want, want_pivot = cases.numpy_ic0(n, rp, ci, va)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=name)
        assert pivot == want_pivot == -1
        assert not np.array_equal(_bits(got), _bits(va))                # it did factor something
        # the upper positions are the transposed lower bits
        np.testing.assert_array_equal(_bits(got[cases.transposed_positions(n, rp, ci)]), _bits(got), err_msg=name)
        # only A's lower triangle and diagonal are read
        upper = ci > cases.rows_of(n, rp)
        junk = va.copy()
        junk[upper] = np.float32(1e30)
        J = spmv.csr_from_arrays(n, n, rp, ci, junk)
        np.testing.assert_array_equal(_bits(spmv.ic0_cpu_csr(J)[0]), _bits(want), err_msg=name)
        spmv.csr_destroy(J)
        # in place through the C ABI: l_values is A's own host array
        H = spmv.csr_from_arrays(n, n, rp, ci, va.copy())
        host_values = ctypes.cast(H.contents.values, ctypes.c_void_p)
        assert spmv.lib().spmv_c_ic0_cpu_csr(H, host_values, None) == 0
        np.testing.assert_array_equal(_bits(np.ctypeslib.as_array(H.contents.values, shape=(ci.size,))), _bits(want))
        spmv.csr_destroy(H)
        spmv.csr_destroy(A)


def test_exact_factors_come_back_exactly(spmv):
    for seed in (0, 2):
        n, rp, ci, va, fact = cases.exact_tridiagonal(257, seed)
        proven = cases.prove_exact(n, rp, ci, va)
        np.testing.assert_array_equal(_bits(proven), _bits(fact))       # the bidiagonal it was built from
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        got, pivot = spmv.ic0_cpu_csr(A)
        np.testing.assert_array_equal(_bits(got), _bits(fact))
        assert pivot == -1
        spmv.csr_destroy(A)
    n, rp, ci, va = cases.arrow_spd(70)
    proven = cases.prove_exact(n, rp, ci, va, shift=6)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    got, pivot = spmv.ic0_cpu_csr(A)
    np.testing.assert_array_equal(_bits(got), _bits(proven))
    assert pivot == -1 and got[-1] == 64.0 and not np.array_equal(got[rp[n - 1]:], va[rp[n - 1]:])
    spmv.csr_destroy(A)


# ---- pivots --------------------------------------------------------------------------------------------------
def test_bad_pivot_is_reported_and_is_not_an_error(spmv, spd):
    dense_cases = {
        # row 2: w_22 = 1/4 - (1/2)^2 - l_21^2 < 0, l_22 = NaN, and row 3 inherits it: the lowest bad row is 2
        "indefinite at row 2": ([[4, 1, 1, 0], [1, 4, 1, 0], [1, 1, .25, 1], [0, 0, 1, 4]], 2),
        # l_10 = 2 / 2 = 1, w_11 = 1 - 1 = 0: l_11 = 0 exactly, and row 2 divides by it
        "zero pivot at row 1": ([[4, 2, 0], [2, 1, 1], [0, 1, 4]], 1),
        "clean": ([[4, 1, 0], [1, 4, 1], [0, 1, 4]], -1),
    }
    for name, (dense, want) in dense_cases.items():
        dense = np.asarray(dense, np.float32)
        n = dense.shape[0]
        rows, cols = np.nonzero(dense)
        _, rp, ci, va = cases.csr_from_coo(n, rows, cols, dense[rows, cols])
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        with np.errstate(all="ignore"):
            got, pivot = spmv.ic0_cpu_csr(A)
            ref, ref_pivot = cases.numpy_ic0(n, rp, ci, va)
        assert pivot == ref_pivot == want, name
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=name)
        np.testing.assert_array_equal(_bits(got)[~np.isnan(ref)], _bits(ref)[~np.isnan(ref)], err_msg=name)
        spmv.csr_destroy(A)
    # one row of a larger matrix made indefinite: the lowest bad row is that one
    n, rp, ci, va = spd.poisson2d(12)
    va = va.copy()
    va[(cases.rows_of(n, rp) == 77) & (ci == 77)] = -4.0
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    with np.errstate(all="ignore"):
        got, pivot = spmv.ic0_cpu_csr(A)
        ref, ref_pivot = cases.numpy_ic0(n, rp, ci, va)
    assert pivot == ref_pivot == 77 and np.isnan(got).any()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    spmv.csr_destroy(A)


# ---- rejections ----------------------------------------------------------------------------------------------
def _cpu_rejects(spmv, n, cols, rp, ci, va, code):
    A = spmv.csr_from_arrays(n, cols, rp, ci, va)
    out = np.full(max(len(va), 1), -77.0, np.float32)
    pivot = ctypes.c_int32(55)
    status = spmv.lib().spmv_c_ic0_cpu_csr(A, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pivot))
    assert status == code and (out == -77.0).all()
    with pytest.raises(ValueError):
        spmv.ic0_cpu_csr(A)
    spmv.csr_destroy(A)


# (rows, row_ptrs, col_indices, values, error name): shared with test_gpu_ic0.py
REJECTED = {
    "unsorted row": (3, [0, 2, 4, 6], [0, 1, 1, 0, 1, 2], [4, 1, 4, 1, 1, 4], "INVALID_ARGUMENT"),
    "repeated column": (3, [0, 2, 5, 6], [0, 1, 0, 1, 1, 2], [4, 1, 1, 2, 2, 4], "INVALID_ARGUMENT"),
    "missing diagonal": (3, [0, 2, 3, 5], [0, 1, 0, 1, 2], [4, 1, 1, 1, 4], "INVALID_ARGUMENT"),
    "lower entry without its upper": (3, [0, 1, 3, 5], [0, 0, 1, 1, 2], [4, 1, 4, 1, 4], "INVALID_ARGUMENT"),
    "upper entry without its lower": (3, [0, 2, 3, 4], [0, 2, 1, 2], [4, 1, 4, 4], "INVALID_ARGUMENT"),
    "column out of range": (3, [0, 2, 4, 6], [0, 1, 0, 1, 1, 7], [4, 1, 1, 4, 1, 4], "INVALID_FORMAT"),
    "row_ptrs decrease": (3, [0, 4, 2, 6], [0, 1, 0, 1, 1, 2], [4, 1, 1, 4, 1, 4], "INVALID_FORMAT"),
}


def test_cpu_rejections_leave_the_output_untouched(spmv):
    E = spmv.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    for name, (n, rp, ci, va, code) in REJECTED.items():
        _cpu_rejects(spmv, n, n, rp, ci, f32(va), getattr(E, code))
    _cpu_rejects(spmv, 2, 3, [0, 1, 2], [0, 1], f32([4, 4]), E.INVALID_DIMENSION)
    # malformed arrays come before the sorting rule: an unsorted row that also holds column 7
    _cpu_rejects(spmv, 3, 3, [0, 2, 4, 6], [0, 1, 1, 0, 1, 7], f32([4, 1, 4, 1, 1, 4]), E.INVALID_FORMAT)
    # nulls
    lib = spmv.lib()
    A = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], f32([4, 4]))
    out = np.zeros(2, np.float32)
    assert lib.spmv_c_ic0_cpu_csr(None, out.ctypes.data_as(ctypes.c_void_p), None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_ic0_cpu_csr(A, None, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_ic0_cpu_csr(A, out.ctypes.data_as(ctypes.c_void_p), None) == 0      # bad_pivot may be NULL
    assert (out == 2.0).all()
    spmv.csr_destroy(A)
    Z = spmv.csr_create(0, 0, 0)
    pivot = ctypes.c_int32(9)
    assert lib.spmv_c_ic0_cpu_csr(Z, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(pivot)) == 0
    assert pivot.value == -1
    spmv.csr_destroy(Z)


def _c_call(spmv, A, l):
    out = spmv.IC0Result(error_code=12345, bad_pivot=99)
    rc = spmv.lib().spmv_c_ic0_csr(A, ctypes.c_void_p(l), ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_device_entry_checks_in_the_stated_order_before_any_device_work(spmv):
    E = spmv.SpMVError
    for call in (lambda A, l: _c_call(spmv, A, l), lambda A, l: spmv.ic0_csr(A, l),
                 lambda A, l: spmv.IC0Result(error_code=spmv.lib().spmv_c_ic0_csr_async(A, ctypes.c_void_p(l), None))):
        # 1. nulls
        assert call(None, L).error_code == E.INVALID_ARGUMENT
        R = spmv.csr_create(5, 4, 0)
        assert call(R, None).error_code == E.INVALID_ARGUMENT
        # 2. not square, before the empty and format checks
        assert call(R, L).error_code == E.INVALID_DIMENSION
        spmv.csr_destroy(R)
        # 3. no rows: SUCCESS
        Z = spmv.csr_create(0, 0, 0)
        res = call(Z, L)
        assert (res.error_code, res.num_levels, res.launches) == (E.SUCCESS, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (a host-only matrix; a wrap without columns)
        H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], np.asarray([4, 4], np.float32))
        assert call(H, L).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(H)
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
        assert call(D, FAKE_VA + 4).error_code == E.INVALID_FORMAT       # before the overlap check
        spmv.csr_destroy(D)
        # 5. partial overlap with A's values (16 floats = 64 bytes); the same array is checked later, not here
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
        for l in (FAKE_VA + 4, FAKE_VA + 60, FAKE_VA - 60, FAKE_VA - 4):
            assert call(D, l).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
    out = spmv.IC0Result(error_code=7, num_levels=9)
    assert spmv.lib().spmv_c_ic0_csr(None, ctypes.c_void_p(L), ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and out.num_levels == 0 and out.bad_pivot == -1
    assert spmv.lib().spmv_c_ic0_csr(None, ctypes.c_void_p(L), None) == E.INVALID_ARGUMENT      # out may be NULL


def test_cg_solve_ic_checks_before_any_device_work(spmv):
    E = spmv.SpMVError
    D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    F = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, L)
    code = lambda *a: spmv.cg_solve_ic(*a).error_code
    R = spmv.csr_create(5, 4, 0)
    S9 = spmv.csr_wrap_device(9, 9, 16, FAKE_RP, FAKE_CI, L)
    Z = spmv.csr_create(0, 0, 0)
    H = spmv.csr_from_arrays(8, 8, np.arange(9, dtype=np.int32), np.arange(8, dtype=np.int32), np.ones(8, np.float32))
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    # cg_solve's checks first, in its order: nulls, A's dimensions, the empty system, A's arrays, the config, overlap
    assert code(None, F, B, X) == E.INVALID_ARGUMENT
    assert code(D, F, None, X) == E.INVALID_ARGUMENT
    assert code(D, F, B, None) == E.INVALID_ARGUMENT
    assert code(R, None, B, X) == E.INVALID_DIMENSION
    res = spmv.cg_solve_ic(Z, None, B, X)
    assert (res.error_code, res.converged, res.iterations) == (0, 1, 0)
    assert code(H, None, B, X, bad_cfg) == E.INVALID_FORMAT
    assert code(D, None, B, X, bad_cfg) == E.INVALID_ARGUMENT
    assert code(D, None, B, X, spmv.CGConfig(max_iterations=-1)) == E.INVALID_ARGUMENT
    assert code(D, None, B, X, spmv.CGConfig(engine=2)) == E.INVALID_ARGUMENT
    assert code(D, R, B, B + 4) == E.INVALID_ARGUMENT
    # then the factor: null, its dimensions (not square; another size), its arrays; the preconditioner is not read
    for cfg in (None, spmv.CGConfig(preconditioner=2)):
        assert code(D, None, B, X, cfg) == E.INVALID_ARGUMENT
        assert code(D, R, B, X, cfg) == E.INVALID_DIMENSION
        assert code(D, S9, B, X, cfg) == E.INVALID_DIMENSION
        assert code(D, H, B, X, cfg) == E.INVALID_FORMAT
    # cg_solve itself still rejects an unknown preconditioner
    assert spmv.cg_solve(D, B, X, spmv.CGConfig(preconditioner=2)).error_code == E.INVALID_ARGUMENT
    out = spmv.CGResult(error_code=7, iterations=9)
    assert spmv.lib().spmv_c_cg_solve_ic(D, None, ctypes.c_void_p(B), ctypes.c_void_p(X), None,
                                         ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and out.iterations == 0
    assert spmv.lib().spmv_c_cg_solve_ic(D, None, ctypes.c_void_p(B), ctypes.c_void_p(X), None,
                                         None) == E.INVALID_ARGUMENT
    for M in (D, F, R, S9, Z, H):
        spmv.csr_destroy(M)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_ic0_cpu_csr_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-ic0 builds tests/cpp/bin/ic0_host_sanitized (csrc/factor0_host.cpp and
    tests/cpp/ic0_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-ic0"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "ic0_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
