"""The factorised sparse approximate inverse (include/spmv/fsai.h) on the host side (no GPU): the exported names and the
struct layout; fsai_cpu_csr against the restatement of the header in tests/fsai_cases.py at zero tolerance; the exact
tier against the Fraction inverse; the unit diagonal of G A G^T; every rejection on host arrays with G untouched; the
argument checks of the device entry points, which come before any device work; the reported bad row; and
csrc/fsai_host.cpp under AddressSanitizer + UBSan through a stand-alone caller."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import fsai_cases as fc
import ic0_cases
from conftest import ROOT

spd = importlib.import_module("gpu-spmv_amd.spd")

FAKE_RP, FAKE_CI, FAKE_VA = 0x800000, 0x900000, 0xA00000          # fake, never-dereferenced device addresses
FAKE_B, FAKE_X = 0x500000, 0x600000
NAMES = ("fsai_csr", "fsai_csr_numeric", "fsai_cpu_csr")


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _with_pattern(matrix, make_pattern):
    n, rp, ci, va = matrix
    return n, rp, ci, va, make_pattern(n, rp, ci)


# name -> (n, rp, ci, va, pattern or None); small enough for the entry-by-entry restatement
CASES = {
    "n=1": lambda: (1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0], np.float32), None),
    "dense_spd_block(20)": lambda: fc.dense_spd_block(20) + (None,),
    "banded_spd(40,4)": lambda: fc.banded_spd(40, 4) + (None,),
    "sorted_random_spd(120,8)": lambda: ic0_cases.sorted_random_spd(120, 8, 11) + (None,),
    "poisson2d(8)": lambda: spd.poisson2d(8) + (None,),
    "poisson3d(4)": lambda: spd.poisson3d(4) + (None,),
    "poisson2d(8), S = I": lambda: _with_pattern(spd.poisson2d(8), lambda n, rp, ci: fc.identity_pattern(n)),
    "banded_spd(40,4), S = its band of 1": lambda: _with_pattern(fc.banded_spd(40, 4),
                                                                lambda n, rp, ci: fc.band_of(n, rp, ci, 1)),
    "poisson2d(8), S = A*A": lambda: _with_pattern(spd.poisson2d(8), fc.squared_pattern),
    "poisson3d(4), S = A*A": lambda: _with_pattern(spd.poisson3d(4), fc.squared_pattern),
}


def host_fsai(spmv, n, rp, ci, va, pattern=None):
    """(status, bad_row, (g_rp, g_ci, g_values) or None) of fsai_cpu_csr; S carries values that are never read"""
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    S = None if pattern is None else spmv.csr_from_arrays(n, n, pattern[0], pattern[1],
                                                          np.full(len(pattern[1]), np.nan, np.float32))
    G = spmv.csr_create(1, 1, 0)
    status, bad = spmv.fsai_cpu_csr(G, A, S)
    got = None
    if status == 0:
        m = G.contents
        assert (m.num_rows, m.num_cols) == (n, n) and m.owns_host_memory and not m.d_row_ptrs
        got = spmv.csr_host_arrays(G)
        assert m.nnz == got[1].size
    else:
        assert (G.contents.num_rows, G.contents.num_cols, G.contents.nnz) == (1, 1, 0)
    for M in (A, S, G):
        spmv.csr_destroy(M)
    return status, bad, got


def test_names_exist_in_the_headers_the_library_and_python(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    public = open(os.path.join(ROOT, "include", "spmv", "fsai.h")).read()
    cg = open(os.path.join(ROOT, "include", "spmv", "cg.h")).read()
    for name in NAMES + ("cg_solve_fsai",):
        assert "spmv_c_" + name in spmv.EXPORTED_SYMBOLS and hasattr(spmv.lib(), "spmv_c_" + name), name
        assert "spmv_c_" + name + "(" in header and callable(getattr(spmv, name)), name
        assert " " + name + "(" in (cg if name == "cg_solve_fsai" else public), name
    for word in ("struct FSAIResult", "bit for bit", "fsai_lanes", "fsai_class", "long_row", "bad_row"):
        assert word in public
    assert "spmv_c_fsai_result" in header


def test_struct_size_and_offsets(spmv):
    R = spmv.FSAIResult
    assert ctypes.sizeof(R) == 32
    assert [f for f, _ in R._fields_] == ["error_code", "nnz", "max_row", "row_class", "lanes_per_row", "bad_row",
                                          "long_row", "elapsed_ms"]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


@pytest.mark.parametrize("name", list(CASES))
def test_fsai_cpu_csr_is_the_restatement_bit_for_bit(spmv, name):
    n, rp, ci, va, pattern = CASES[name]()
    want_rp, want_ci, want, want_bad = fc.numpy_fsai(n, rp, ci, va, pattern)
    status, bad, (g_rp, g_ci, g) = host_fsai(spmv, n, rp, ci, va, pattern)
    assert (status, bad, want_bad) == (0, -1, -1)
    np.testing.assert_array_equal(g_rp, want_rp)
    np.testing.assert_array_equal(g_ci, want_ci)
    np.testing.assert_array_equal(bits(g), bits(want))
    # lower triangular, rows sorted, the diagonal last
    rows = fc.rows_of(n, g_rp)
    assert (g_ci <= rows).all() and (g_ci[g_rp[1:] - 1] == np.arange(n)).all()
    assert all((np.diff(g_ci[g_rp[i]:g_rp[i + 1]]) > 0).all() for i in range(n))
    # G A G^T has a unit diagonal: the restatement gave 2e-16 before the fp32 store, the bound is fp32 rounding of g
    error = fc.unit_diagonal_error(n, rp, ci, va, g_rp, g_ci, g)
    print(f"{name}: max |diag(G A G^T) - 1| = {error:.3e}")
    assert error <= 1e-5
    if name.endswith("S = I"):                 # G = diag(1 / sqrt(a_ii)), correctly rounded through the rule
        d = va[ci == fc.rows_of(n, rp)].astype(np.float64)
        np.testing.assert_array_equal(bits(g), bits((1.0 / np.sqrt(d)).astype(np.float32)))
    if "A*A" in name:                          # the pattern is richer than A: M has absent entries
        assert g_ci.size > fc.lower_pattern(n, rp, ci)[1].size


def test_upper_values_of_a_are_never_read(spmv):
    n, rp, ci, va = fc.banded_spd(40, 4)
    _, _, want = host_fsai(spmv, n, rp, ci, va)
    changed = va.copy()
    changed[ci > fc.rows_of(n, rp)] = np.nan
    _, bad, got = host_fsai(spmv, n, rp, ci, changed)
    assert bad == -1
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]))


@pytest.mark.parametrize("sizes", [(1, 2, 3, 4, 5, 6), (6, 6, 5, 1, 6)])
def test_the_exact_tier_is_the_fraction_inverse(spmv, sizes):
    n, rp, ci, va, L = fc.exact_blocks(sizes)
    want = fc.prove_exact(n, rp, ci, va, L)
    status, bad, (g_rp, g_ci, g) = host_fsai(spmv, n, rp, ci, va)
    assert (status, bad) == (0, -1)
    np.testing.assert_array_equal(bits(g), bits(want))
    np.testing.assert_array_equal(bits(fc.numpy_fsai(n, rp, ci, va)[2]), bits(want))
    dense = np.zeros((n, n))
    dense[fc.rows_of(n, g_rp), g_ci] = g
    np.testing.assert_array_equal(dense @ L, np.eye(n))            # exactly: every product and sum is a small dyadic


def test_bad_row_on_an_indefinite_matrix(spmv):
    n, rp, ci, va = fc.indefinite(40, 17)
    _, _, _, want_bad = fc.numpy_fsai(n, rp, ci, va)
    status, bad, (g_rp, _, g) = host_fsai(spmv, n, rp, ci, va)
    assert (status, bad, want_bad) == (0, 17, 17)
    assert np.isnan(g[g_rp[18] - 1]) and np.isfinite(g[:g_rp[17]]).all()


def _bad(matrix, **change):
    """(n, rp, ci, va) with row pointers or columns overwritten at the given positions"""
    n, rp, ci, va = matrix
    rp, ci = rp.copy(), ci.copy()
    for where, value in change.get("rp", {}).items():
        rp[where] = value
    for where, value in change.get("ci", {}).items():
        ci[where] = value
    return n, rp, ci, va


def rejected():
    """name -> (A's arrays, the pattern or None, error name); shared with test_gpu_fsai.py"""
    good = fc.banded_spd(6, 1)                  # rows 0: [0 1], 1: [0 1 2], ... nnz 16
    n, rp, ci, va = good
    pattern = (rp, ci)
    out = {
        "A: column past n": (_bad(good, ci={4: 9}), None, "INVALID_FORMAT"),
        "A: negative column": (_bad(good, ci={4: -1}), None, "INVALID_FORMAT"),
        "A: row pointers decrease": (_bad(good, rp={2: 1}), None, "INVALID_FORMAT"),
        "A: row pointer past nnz": (_bad(good, rp={6: 40}), None, "INVALID_FORMAT"),
        "A: negative row pointer": (_bad(good, rp={0: -1}), None, "INVALID_FORMAT"),
        "S: column past n": (good, _bad(good, ci={4: 9})[1:3], "INVALID_FORMAT"),
        "S: row pointers decrease": (good, _bad(good, rp={2: 1})[1:3], "INVALID_FORMAT"),
        "S: row pointer past nnz": (good, _bad(good, rp={6: 40})[1:3], "INVALID_FORMAT"),
        "A: a row descends": (_bad(good, ci={2: 2, 4: 0}), None, "INVALID_ARGUMENT"),
        "A: a column repeats": (_bad(good, ci={3: 0}), pattern, "INVALID_ARGUMENT"),
        "S: a row descends": (good, _bad(good, ci={2: 2, 4: 0})[1:3], "INVALID_ARGUMENT"),
        "S: no (3,3)": (good, (np.array([0, 1, 2, 3, 4, 5, 6], np.int32), np.array([0, 1, 2, 2, 4, 5], np.int32)),
                        "INVALID_ARGUMENT"),
        "S: an empty row": (good, (np.array([0, 1, 2, 2, 3, 4, 5], np.int32), np.array([0, 1, 3, 4, 5], np.int32)),
                            "INVALID_ARGUMENT"),
    }
    return out


def test_host_rejections_leave_g_untouched(spmv):
    E = spmv.SpMVError
    for name, (matrix, pattern, code) in rejected().items():
        status, _, got = host_fsai(spmv, *matrix, pattern)
        assert status == getattr(E, code) and got is None, name
    # a pattern row of 65 entries, and the same matrix under a sparser pattern that is fine
    n, rp, ci, va = fc.dense_spd_block(65)
    assert host_fsai(spmv, n, rp, ci, va)[0] == E.INVALID_ARGUMENT
    assert host_fsai(spmv, n, rp, ci, va, fc.band_of(n, rp, ci, 63))[0] == 0
    # shapes, nulls, aliases, missing host arrays
    n, rp, ci, va = fc.banded_spd(6, 1)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    G = spmv.csr_create(1, 1, 0)
    R = spmv.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], [4.0, 4.0])
    small = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], [4.0, 4.0])
    D = spmv.csr_wrap_device(n, n, int(ci.size), FAKE_RP, FAKE_CI, FAKE_VA)            # no host arrays
    Z = spmv.csr_create(0, 0, 0)
    f = spmv.fsai_cpu_csr
    assert f(None, A)[0] == E.INVALID_ARGUMENT and f(G, None)[0] == E.INVALID_ARGUMENT
    assert f(A, A)[0] == E.INVALID_ARGUMENT and f(small, A, small)[0] == E.INVALID_ARGUMENT
    assert f(G, R)[0] == E.INVALID_DIMENSION and f(G, A, R)[0] == E.INVALID_DIMENSION
    assert f(G, A, small)[0] == E.INVALID_DIMENSION
    assert f(G, D)[0] == E.INVALID_FORMAT and f(G, A, D)[0] == E.INVALID_FORMAT
    assert (G.contents.num_rows, G.contents.num_cols, G.contents.nnz) == (1, 1, 0)
    assert f(G, Z) == (0, -1) and (G.contents.num_rows, G.contents.nnz) == (0, 0)      # no rows: an empty G
    for M in (A, G, R, small, D, Z):
        spmv.csr_destroy(M)


def test_device_entry_points_check_before_any_device_work(spmv):
    """every call below must return before it touches a (fake) device address"""
    E = spmv.SpMVError
    wrap = spmv.csr_wrap_device
    A = wrap(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    other = wrap(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    G = spmv.csr_create(1, 1, 0)
    wide = wrap(8, 9, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    small = wrap(7, 7, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    host_only = spmv.csr_from_arrays(8, 8, np.arange(9), np.arange(8), np.ones(8, np.float32))
    missing = [wrap(8, 8, 16, None, FAKE_CI, FAKE_VA), wrap(8, 8, 16, FAKE_RP, None, FAKE_VA)]
    no_values = wrap(8, 8, 16, FAKE_RP, FAKE_CI, None)
    empty = spmv.csr_create(0, 0, 0)
    code = lambda res: res.error_code

    assert code(spmv.fsai_csr(None, A)) == E.INVALID_ARGUMENT and code(spmv.fsai_csr(G, None)) == E.INVALID_ARGUMENT
    assert code(spmv.fsai_csr(A, A)) == E.INVALID_ARGUMENT
    assert code(spmv.fsai_csr(other, A, other)) == E.INVALID_ARGUMENT
    assert code(spmv.fsai_csr(G, wide)) == E.INVALID_DIMENSION
    assert code(spmv.fsai_csr(G, A, wide)) == E.INVALID_DIMENSION
    assert code(spmv.fsai_csr(G, A, small)) == E.INVALID_DIMENSION
    for M in missing + [no_values, host_only]:
        assert code(spmv.fsai_csr(G, M)) == E.INVALID_FORMAT
    for M in missing + [host_only]:             # only S's structure arrays are needed
        assert code(spmv.fsai_csr(G, A, M)) == E.INVALID_FORMAT
    res = spmv.fsai_csr(G, wide)
    assert (res.nnz, res.max_row, res.row_class, res.lanes_per_row, res.bad_row, res.long_row) == (0, 0, 0, 0, -1, -1)
    assert (G.contents.num_rows, G.contents.num_cols, G.contents.nnz) == (1, 1, 0) and not G.contents.d_row_ptrs

    numeric = spmv.fsai_csr_numeric
    assert code(numeric(None, A)) == E.INVALID_ARGUMENT and code(numeric(other, None)) == E.INVALID_ARGUMENT
    assert code(numeric(A, A)) == E.INVALID_ARGUMENT
    assert code(numeric(other, wide)) == E.INVALID_DIMENSION and code(numeric(wide, A)) == E.INVALID_DIMENSION
    assert code(numeric(small, A)) == E.INVALID_DIMENSION
    for M in missing + [no_values, host_only]:
        assert code(numeric(M, A)) == E.INVALID_FORMAT and code(numeric(other, M)) == E.INVALID_FORMAT
    also_empty = spmv.csr_create(0, 0, 0)
    assert code(numeric(empty, also_empty)) == 0                                        # nothing to do

    # cg_solve_fsai: cg_solve's checks first, in their order, then G and GT
    solve = lambda *a, **k: spmv.cg_solve_fsai(*a, **k).error_code
    assert solve(None, other, other, FAKE_B, FAKE_X) == E.INVALID_ARGUMENT
    assert solve(A, other, other, None, FAKE_X) == E.INVALID_ARGUMENT
    assert solve(A, other, other, FAKE_B, None) == E.INVALID_ARGUMENT
    assert solve(wide, None, None, FAKE_B, FAKE_X) == E.INVALID_DIMENSION
    assert solve(missing[0], None, None, FAKE_B, FAKE_X) == E.INVALID_FORMAT
    assert solve(A, None, None, FAKE_B, FAKE_X, spmv.CGConfig(tolerance=-1.0)) == E.INVALID_ARGUMENT
    assert solve(A, other, wide, FAKE_B, FAKE_B) == E.INVALID_ARGUMENT                  # b and x overlap
    assert solve(A, None, other, FAKE_B, FAKE_X) == E.INVALID_ARGUMENT
    assert solve(A, other, None, FAKE_B, FAKE_X) == E.INVALID_ARGUMENT
    assert solve(A, wide, other, FAKE_B, FAKE_X) == E.INVALID_DIMENSION
    assert solve(A, other, small, FAKE_B, FAKE_X) == E.INVALID_DIMENSION
    for M in missing + [no_values, host_only]:
        assert solve(A, M, other, FAKE_B, FAKE_X) == E.INVALID_FORMAT
        assert solve(A, other, M, FAKE_B, FAKE_X) == E.INVALID_FORMAT
    # config.preconditioner is not read
    assert solve(A, other, None, FAKE_B, FAKE_X, spmv.CGConfig(preconditioner=7)) == E.INVALID_ARGUMENT
    assert solve(A, wide, other, FAKE_B, FAKE_X, spmv.CGConfig(preconditioner=7)) == E.INVALID_DIMENSION
    for M in [A, other, G, wide, small, host_only, no_values, empty, also_empty] + missing:
        spmv.csr_destroy(M)


def test_fsai_host_under_sanitizers():
    """make -C gpu-spmv_amd sanitize-fsai builds tests/cpp/bin/fsai_host_sanitized (csrc/fsai_host.cpp and
    tests/cpp/fsai_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-fsai"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "fsai_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
