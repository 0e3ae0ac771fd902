"""Matrix assembly (include/spmv/assemble.h) on the host side (no GPU): the exported names and struct layouts;
csr_from_coo_cpu against the restatement of the header in tests/assemble_cases.py at zero tolerance on every case the
device tests use, in both modes; the restatement against a dictionary-of-lists accumulation; the round trip through
csr_from_dense; the argument checks that come before any device work; and csrc/assemble_host.cpp under
AddressSanitizer + UBSan through a stand-alone caller."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import assemble_cases as ac
from conftest import ROOT

ROWS, COLS, VALS = 0x500000, 0x600000, 0x700000          # fake, never-dereferenced device addresses
FAKE_RP, FAKE_CI, FAKE_VA = 0x800000, 0x900000, 0xA00000
NAMES = ("csr_from_coo_cpu", "csr_from_coo_gpu", "csr_coo_refill", "csr_coo_refill_async", "coo_plan_destroy",
         "coo_plan_info", "csr_row_indices_gpu")


def tile_entries(spmv):
    """the device sort's geometry, reported by every call: this one fails its first check and touches no device"""
    res = spmv.csr_from_coo_gpu(None, 1, 1, 0, None, None, None)
    assert res.error_code == spmv.SpMVError.INVALID_ARGUMENT and res.tile_entries >= 256
    return res.tile_entries


@pytest.fixture(scope="module")
def cases(spmv):
    return ac.cases(tile_entries(spmv))


CASE_NAMES = list(ac.cases(4096))          # the names do not depend on the tile, only the sizes behind them


def host_assemble(spmv, case, mode):
    num_rows, num_cols, rows, cols, vals = case
    C = spmv.csr_create(2, 2, 1)
    status = spmv.csr_from_coo_cpu(C, num_rows, num_cols, rows, cols, vals, spmv.CooConfig(duplicates=mode))
    assert status == 0
    m = C.contents
    assert (m.num_rows, m.num_cols) == (num_rows, num_cols) and m.owns_host_memory
    got = spmv.csr_host_arrays(C)
    assert m.nnz == got[1].size
    spmv.csr_destroy(C)
    return got


def test_names_exist_in_the_headers_the_library_and_python(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    public = open(os.path.join(ROOT, "include", "spmv", "assemble.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in spmv.EXPORTED_SYMBOLS and hasattr(spmv.lib(), "spmv_c_" + name), name
        assert "spmv_c_" + name + "(" in header and callable(getattr(spmv, name)), name
        assert " " + name + "(" in public, name
    for word in ("struct CooConfig", "struct CooResult", "struct CooPlan", "COO_SUM", "COO_KEEP", "tile_entries"):
        assert word in public
    assert (spmv.COO_SUM, spmv.COO_KEEP) == (0, 1) == (spmv.CooConfig.COO_SUM, spmv.CooConfig.COO_KEEP)


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R = spmv.CooConfig, spmv.CooResult
    assert ctypes.sizeof(C) == 8 and ctypes.sizeof(R) == 28
    assert [f for f, _ in C._fields_] == ["duplicates", "reserved"]
    assert [f for f, _ in R._fields_] == ["error_code", "nnz_out", "combined", "passes", "tile_entries", "launches",
                                          "elapsed_ms"]
    assert [getattr(C, f).offset for f, _ in C._fields_] == [0, 4]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24]
    c = C()
    assert (c.duplicates, c.reserved) == (0, 0)
    assert tile_entries(spmv) % 64 == 0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_csr_from_coo_cpu_is_the_restatement(spmv, cases, name):
    case = cases[name]()
    for mode in ac.MODES:
        got = host_assemble(spmv, case, mode)
        want = ac.assemble(*case, mode=mode)
        assert ac.same(got, want), (name, mode)
        if mode == ac.KEEP:
            assert got[1].size == len(case[2])
    # the default config is COO_SUM
    C = spmv.csr_create(0, 0, 0)
    assert spmv.csr_from_coo_cpu(C, *case) == 0
    assert ac.same(spmv.csr_host_arrays(C), ac.assemble(*case))
    spmv.csr_destroy(C)


@pytest.mark.parametrize("name", ["n=257", "three keys", "run from slot 63", "1e8, 1, -1e8", "special values",
                                  "empty first and last rows", "1000 empty rows", "1 x 1"])
def test_the_restatement_is_a_dictionary_of_lists_accumulation(cases, name):
    """the stable lexsort visits every cell's contributions in source order: the same values, bit for bit, as
    A[i, j] += v over the triplets as they come, with the cells read out in (row, column) order"""
    case = cases[name]()
    rp, ci, va, sources = ac.by_dictionary(*case)
    assert ac.same(ac.assemble(*case), (rp, ci, va))
    assert all(places == sorted(places) for places in sources)
    # and COO_KEEP lists exactly those source positions, run after run
    keep = ac.assemble(*case, mode=ac.KEEP)
    flat = np.concatenate([np.asarray(p) for p in sources]) if sources else np.empty(0, int)
    assert np.array_equal(ac.bits(keep[2]), ac.bits(np.asarray(case[4])[flat]))


def test_order_matters_in_the_cancelling_runs(cases):
    """the case is worth its name: summing each run in another order changes bits"""
    case = cases["1e8, 1, -1e8"]()
    forward = ac.assemble(*case)
    num_rows, num_cols, rows, cols, vals = case
    backward = ac.assemble(num_rows, num_cols, rows[::-1], cols[::-1], vals[::-1])
    assert np.array_equal(forward[1], backward[1]) and not np.array_equal(ac.bits(forward[2]), ac.bits(backward[2]))


def test_round_trip_through_csr_from_dense(spmv):
    rng = np.random.default_rng(3)
    dense = np.where(rng.random((37, 53)) < 0.2, rng.standard_normal((37, 53)), 0.0).astype(np.float32)
    A = spmv.csr_create(0, 0, 0)
    assert spmv.csr_from_dense(A, dense, 37, 53) == 0
    rp, ci, va = spmv.csr_host_arrays(A)
    rows = np.repeat(np.arange(37, dtype=np.int32), np.diff(rp))
    p = rng.permutation(ci.size)
    for mode in ac.MODES:
        C = spmv.csr_create(0, 0, 0)
        assert spmv.csr_from_coo_cpu(C, 37, 53, rows[p], ci[p], va[p], spmv.CooConfig(duplicates=mode)) == 0
        assert ac.same(spmv.csr_host_arrays(C), (rp, ci, va))
        assert np.array_equal(spmv.csr_to_dense(C), dense)
        spmv.csr_destroy(C)
    spmv.csr_destroy(A)


def test_host_rejections(spmv):
    E = spmv.SpMVError
    rows, cols, vals = [0, 1, 2], [2, 1, 0], [1.0, 2.0, 3.0]
    C = spmv.csr_create(1, 1, 0)
    call = spmv.csr_from_coo_cpu
    assert call(None, 3, 3, rows, cols, vals) == E.INVALID_ARGUMENT
    assert call(C, 3, 3, None, cols, vals, n=3) == E.INVALID_ARGUMENT
    assert call(C, 3, 3, rows, None, vals) == E.INVALID_ARGUMENT
    assert call(C, 3, 3, rows, cols, None) == E.INVALID_ARGUMENT
    assert call(C, -1, 3, rows, cols, vals) == E.INVALID_DIMENSION
    assert call(C, 3, -1, rows, cols, vals) == E.INVALID_DIMENSION
    assert call(C, 3, 3, rows, cols, vals, n=-1) == E.INVALID_DIMENSION
    # the order of the checks: a null array before a negative size, a negative size before the config
    assert call(C, -1, 3, None, cols, vals, spmv.CooConfig(duplicates=5), n=3) == E.INVALID_ARGUMENT
    assert call(C, -1, 3, rows, cols, vals, spmv.CooConfig(duplicates=5)) == E.INVALID_DIMENSION
    for cfg in (spmv.CooConfig(duplicates=2), spmv.CooConfig(duplicates=-1), spmv.CooConfig(reserved=1)):
        assert call(C, 3, 3, rows, cols, vals, cfg) == E.INVALID_ARGUMENT
    assert call(C, 3, 3, [0, 1, 3], cols, vals) == E.INVALID_FORMAT
    assert call(C, 3, 3, [0, -1, 2], cols, vals) == E.INVALID_FORMAT
    assert call(C, 3, 3, rows, [2, 1, 3], vals) == E.INVALID_FORMAT
    assert call(C, 3, 3, rows, [2, 1, -1], vals) == E.INVALID_FORMAT
    assert call(C, 0, 0, [0], [0], [1.0]) == E.INVALID_FORMAT
    assert (C.contents.num_rows, C.contents.num_cols, C.contents.nnz) == (1, 1, 0)       # as it was
    # nothing to assemble: an all-zero row_ptrs, with and without rows
    assert call(C, 4, 5, [], [], []) == 0 and np.array_equal(spmv.csr_host_arrays(C)[0], [0, 0, 0, 0, 0])
    assert call(C, 0, 0, None, None, None) == 0 and np.array_equal(spmv.csr_host_arrays(C)[0], [0])
    assert (C.contents.num_rows, C.contents.num_cols, C.contents.nnz) == (0, 0, 0)
    spmv.csr_destroy(C)


def test_device_entry_points_check_before_any_device_work(spmv):
    """every call below must return before it touches a (fake) device address"""
    E = spmv.SpMVError
    Cfg = spmv.CooConfig
    C = spmv.csr_create(1, 1, 0)
    build = spmv.csr_from_coo_gpu
    assert build(None, 3, 3, 5, ROWS, COLS, VALS).error_code == E.INVALID_ARGUMENT
    assert build(C, 3, 3, 5, None, COLS, VALS).error_code == E.INVALID_ARGUMENT
    assert build(C, 3, 3, 5, ROWS, None, VALS).error_code == E.INVALID_ARGUMENT
    assert build(C, 3, 3, 5, ROWS, COLS, None).error_code == E.INVALID_ARGUMENT
    assert build(C, -1, 3, 5, ROWS, COLS, VALS).error_code == E.INVALID_DIMENSION
    assert build(C, 3, -1, 5, ROWS, COLS, VALS).error_code == E.INVALID_DIMENSION
    assert build(C, 3, 3, -5, ROWS, COLS, VALS).error_code == E.INVALID_DIMENSION
    assert build(C, -1, 3, 5, None, COLS, VALS, Cfg(reserved=1)).error_code == E.INVALID_ARGUMENT
    assert build(C, -1, 3, 5, ROWS, COLS, VALS, Cfg(reserved=1)).error_code == E.INVALID_DIMENSION
    for cfg in (Cfg(duplicates=2), Cfg(duplicates=-1), Cfg(reserved=1), Cfg(duplicates=1, reserved=7)):
        res, plan = build(C, 3, 3, 5, ROWS, COLS, VALS, cfg, want_plan=True)
        assert res.error_code == E.INVALID_ARGUMENT and plan is None
        assert (res.nnz_out, res.combined, res.passes, res.launches) == (0, 0, 0, 0)
        assert res.tile_entries == tile_entries(spmv)
    assert (C.contents.num_rows, C.contents.num_cols, C.contents.nnz) == (1, 1, 0)
    assert not C.contents.d_row_ptrs
    # csr_row_indices_gpu
    D = spmv.csr_wrap_device(100, 50, 300, FAKE_RP, FAKE_CI, FAKE_VA)
    assert spmv.csr_row_indices_gpu(None, ROWS) == E.INVALID_ARGUMENT
    assert spmv.csr_row_indices_gpu(D, None) == E.INVALID_ARGUMENT
    for rp_, ci_, va_ in ((None, FAKE_CI, FAKE_VA), (FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
        M = spmv.csr_wrap_device(8, 8, 16, rp_, ci_, va_)
        assert spmv.csr_row_indices_gpu(M, ROWS) == E.INVALID_FORMAT
        spmv.csr_destroy(M)
    H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], [1.0, 2.0])                        # host only
    assert spmv.csr_row_indices_gpu(H, ROWS) == E.INVALID_FORMAT
    Z = spmv.csr_create(0, 0, 0)
    assert spmv.csr_row_indices_gpu(Z, None) == 0                                        # nothing to do
    # csr_coo_refill: the null checks (everything else needs a plan, which needs a device)
    for refill in (spmv.csr_coo_refill, spmv.csr_coo_refill_async):
        assert refill(None, D, VALS) == E.INVALID_ARGUMENT
    assert spmv.coo_plan_info(None)[0] == E.INVALID_ARGUMENT
    spmv.coo_plan_destroy(None)                                                          # null-safe
    for X in (C, D, H, Z):
        spmv.csr_destroy(X)


def test_assemble_host_under_sanitizers():
    """make -C gpu-spmv_amd sanitize-assemble builds tests/cpp/bin/assemble_host_sanitized (csrc/assemble_host.cpp and
    tests/cpp/assemble_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-assemble"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "assemble_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
