"""spgemm_csr / spgemm_csr_numeric / spgemm_cpu_csr / spgemm_class_capacity (include/spmv/spgemm.h) on the host side
(no GPU): the exported names and the result layout; spgemm_cpu_csr against a plain double loop in the documented
order, bit for bit, and against an int64 product on small-integer matrices; cancellation, explicit zeros and the
identity; every check that needs no device, in the stated order, with fake device addresses that must never be
dereferenced; the class capacities; and the sanitized caller of spgemm_cpu_csr."""
import ctypes
import os
import re
import subprocess

import numpy as np

import spgemm_cases as sc
from conftest import ROOT

NAMES = ("spgemm_csr", "spgemm_csr_numeric", "spgemm_cpu_csr", "spgemm_class_capacity")
INT_MAX = 2**31 - 1

# fake, never-dereferenced device addresses: every call below must return before it touches them
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


# ---- names and layouts ---------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)                     # what test_host_library.py checks
    cxx = open(os.path.join(ROOT, "include", "spmv", "spgemm.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared and "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name


def test_result_layout(spmv):
    R = spmv.SpGEMMResult
    assert ctypes.sizeof(R) == 104
    names = ["error_code", "nnz", "products", "max_row_products", "max_row_nnz", "symbolic_rows", "numeric_rows",
             "lanes", "symbolic_ms", "numeric_ms"]
    assert [f for f, _ in R._fields_] == names
    assert [getattr(R, f).offset for f in names] == [0, 4, 8, 16, 20, 24, 56, 88, 92, 96]


def test_class_capacities(spmv):
    caps = []
    cls = 1
    while spmv.spgemm_class_capacity(cls) not in (INT_MAX, -1):
        caps.append(spmv.spgemm_class_capacity(cls))
        cls += 1
    assert len(caps) >= 3                                             # at least three LDS tables of growing size
    assert all(a < b for a, b in zip(caps, caps[1:])) and caps[0] >= 1 and caps[-1] < INT_MAX
    assert caps[-1] * 2 * 8 <= 160 * 1024                             # keys + values at load 1/2 fit one workgroup's LDS
    assert spmv.spgemm_class_capacity(cls) == INT_MAX                 # the dense class
    assert spmv.spgemm_class_capacity(cls + 1) == -1 and spmv.spgemm_class_capacity(cls + 7) == -1
    assert spmv.spgemm_class_capacity(0) == -1 and spmv.spgemm_class_capacity(-3) == -1
    assert cls <= 7                                                   # the histograms of SpGEMMResult hold 8 classes


# ---- the arithmetic ------------------------------------------------------------------------------------------
def test_cpu_product_equals_the_plain_double_loop_bit_for_bit(spmv):
    rng = np.random.default_rng(20)
    cases = {}
    cases["37x23 by 23x41"] = (37, 23, 41, sc.random_csr(rng, 37, 23, 0.3), sc.random_csr(rng, 23, 41, 0.3))
    cases["unsorted A with duplicates"] = (29, 17, 33, sc.random_csr(rng, 29, 17, 0.4, sort=False, duplicates=True),
                                           sc.random_csr(rng, 17, 33, 0.35))
    # empty rows in A, rows of A that reference empty rows of B
    a_rows = [[], [(0, 1.5), (2, -2.25)], [], [(1, 3.0)], [(1, 0.5), (3, 7.0)], []]
    b_rows = [[(0, 2.0), (4, -1.0)], [], [(1, 0.75), (4, 0.125), (5, 3.0)], []]
    cases["empty rows"] = (6, 4, 6, sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows))
    empty = lambda r: (np.zeros(r + 1, np.int32), np.empty(0, np.int32), np.empty(0, np.float32))
    cases["A without entries"] = (5, 4, 6, empty(5), sc.csr_from_rows(b_rows))
    cases["B without entries"] = (6, 4, 6, sc.csr_from_rows(a_rows), empty(4))
    cases["no rows"] = (0, 4, 6, empty(0), sc.csr_from_rows(b_rows))
    cases["no columns"] = (6, 4, 0, sc.csr_from_rows(a_rows), empty(4))
    cases["no inner dimension"] = (3, 0, 5, empty(3), empty(0))
    for name, (m, k, n, a, b) in cases.items():
        status, got = sc.host_product(spmv, m, k, n, a, b)
        assert status == 0, name
        want = sc.product_loop(m, n, a, b)
        sc.assert_same(got, want, name)
        assert got[0].size == m + 1
    assert sc.host_product(spmv, *cases["37x23 by 23x41"])[1][1].size > 200           # it did multiply something
    assert sc.host_product(spmv, *cases["B without entries"])[1][1].size == 0


def test_cpu_product_equals_the_int64_product_on_small_integers(spmv):
    rng = np.random.default_rng(21)
    m, k, n = 40, 30, 50
    da = rng.integers(-8, 9, size=(m, k)) * (rng.random((m, k)) < 0.25)
    db = rng.integers(-8, 9, size=(k, n)) * (rng.random((k, n)) < 0.25)
    to_csr = lambda d: sc.csr_from_rows([[(int(c), float(d[i, c])) for c in np.flatnonzero(d[i])]
                                         for i in range(d.shape[0])])
    status, (rp, ci, va) = sc.host_product(spmv, m, k, n, to_csr(da), to_csr(db))
    assert status == 0
    exact = da.astype(np.int64) @ db.astype(np.int64)                 # every partial sum is far below 2^24
    pattern = (da != 0).astype(np.int64) @ (db != 0).astype(np.int64) > 0
    for i in range(m):
        cols = ci[rp[i]:rp[i + 1]]
        np.testing.assert_array_equal(cols, np.flatnonzero(pattern[i]))
        np.testing.assert_array_equal(va[rp[i]:rp[i + 1]].astype(np.int64), exact[i, cols])
    assert (va == 0).any()                                            # cancelled entries are stored


def test_cancellation_and_explicit_zeros_are_kept(spmv):
    # A = [1, -1], B = [[1], [1]]: one stored entry +0.0f
    status, (rp, ci, va) = sc.host_product(spmv, 1, 2, 1, sc.csr_from_rows([[(0, 1.0), (1, -1.0)]]),
                                           sc.csr_from_rows([[(0, 1.0)], [(0, 1.0)]]))
    assert status == 0 and rp.tolist() == [0, 1] and ci.tolist() == [0] and sc.bits(va).tolist() == [0]
    # explicit zeros in A and in B still produce entries; a lone -0.0 product gives +0.0 + -0.0 = +0.0
    a = sc.csr_from_rows([[(0, 0.0), (1, 2.0)], [(1, -0.0)]])
    b = sc.csr_from_rows([[(0, 5.0), (2, 1.0)], [(1, 0.0), (2, 3.0)]])
    status, (rp, ci, va) = sc.host_product(spmv, 2, 2, 3, a, b)
    assert status == 0 and rp.tolist() == [0, 3, 5] and ci.tolist() == [0, 1, 2, 1, 2]
    assert sc.bits(va).tolist() == sc.bits([0.0, 0.0, 6.0, 0.0, 0.0]).tolist()


def test_identity_on_either_side_returns_the_other_factor(spmv):
    rng = np.random.default_rng(22)
    a = sc.random_csr(rng, 31, 19, 0.3)
    eye = lambda r: (np.arange(r + 1, dtype=np.int32), np.arange(r, dtype=np.int32), np.ones(r, np.float32))
    status, got = sc.host_product(spmv, 31, 19, 19, a, eye(19))
    assert status == 0
    sc.assert_same(got, a, "A I")
    status, got = sc.host_product(spmv, 31, 31, 19, eye(31), a)
    assert status == 0
    sc.assert_same(got, a, "I B")


# ---- rejections ----------------------------------------------------------------------------------------------
def _untouched(C):
    m = C.contents
    return (m.num_rows, m.num_cols, m.nnz, bool(m.owns_device_memory), m.d_row_ptrs, m.d_col_indices, m.d_values)


def test_cpu_checks_in_the_stated_order_with_c_untouched(spmv):
    E = spmv.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    A = spmv.csr_from_arrays(2, 3, [0, 2, 3], [0, 2, 1], f32([1, 2, 3]))
    B = spmv.csr_from_arrays(3, 4, [0, 1, 3, 4], [0, 1, 3, 2], f32([1, 2, 3, 4]))
    W = spmv.csr_from_arrays(2, 4, [0, 1, 2], [0, 1], f32([1, 1]))           # 2 rows: wrong inner dimension
    C = spmv.csr_create(2, 3, 0)
    before = _untouched(C)
    lib = spmv.lib()
    assert lib.spmv_c_spgemm_cpu_csr(None, A, B) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spgemm_cpu_csr(C, None, B) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spgemm_cpu_csr(C, A, None) == E.INVALID_ARGUMENT
    assert spmv.spgemm_cpu_csr(A, A, W) == E.INVALID_ARGUMENT                # alias before the dimension check
    assert spmv.spgemm_cpu_csr(W, A, W) == E.INVALID_ARGUMENT
    assert spmv.spgemm_cpu_csr(C, A, W) == E.INVALID_DIMENSION
    bad_b = {
        "two equal adjacent columns": ([0, 1, 3, 4], [0, 1, 1, 2]),
        "one descending pair": ([0, 1, 3, 4], [0, 3, 1, 2]),
        "column out of range": ([0, 1, 3, 4], [0, 1, 4, 2]),
        "negative column": ([0, 1, 3, 4], [0, -1, 3, 2]),
        "row_ptrs decrease": ([0, 3, 1, 4], [0, 1, 3, 2]),
        "row_ptrs do not start at 0": ([1, 1, 3, 4], [0, 1, 3, 2]),
        "row_ptrs do not end at nnz": ([0, 1, 3, 3], [0, 1, 3, 2]),
    }
    for name, (rp, ci) in bad_b.items():
        X = spmv.csr_from_arrays(3, 4, rp, ci, f32([1, 2, 3, 4]))
        assert spmv.spgemm_cpu_csr(C, A, X) == E.INVALID_FORMAT, name
        spmv.csr_destroy(X)
    X = spmv.csr_from_arrays(2, 3, [0, 2, 3], [0, 3, 1], f32([1, 2, 3]))     # A points at B's row 3 of 3
    assert spmv.spgemm_cpu_csr(C, X, B) == E.INVALID_FORMAT
    spmv.csr_destroy(X)
    assert _untouched(C) == before
    # unsorted A with a repeated entry is fine
    X = spmv.csr_from_arrays(2, 3, [0, 3, 4], [2, 0, 2, 1], f32([1, 2, 3, 4]))
    assert spmv.spgemm_cpu_csr(C, X, B) == 0 and C.contents.num_cols == 4 and C.contents.owns_host_memory
    for M in (A, B, W, C, X):
        spmv.csr_destroy(M)


def test_device_entry_checks_in_the_stated_order_before_any_device_work(spmv):
    E = spmv.SpMVError
    A = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    B = spmv.csr_wrap_device(6, 9, 12, FAKE_RP, FAKE_CI, FAKE_VA)
    W = spmv.csr_wrap_device(5, 9, 12, FAKE_RP, FAKE_CI, FAKE_VA)            # wrong inner dimension
    H = spmv.csr_from_arrays(6, 9, np.arange(7, dtype=np.int32), np.arange(6, dtype=np.int32),
                             np.ones(6, np.float32))                         # host only
    NC = spmv.csr_wrap_device(6, 9, 12, FAKE_RP, None, FAKE_VA)              # entries and no columns
    Z = spmv.csr_wrap_device(0, 9, 3, None, FAKE_CI, FAKE_VA)                # no rows cannot hold entries
    C = spmv.csr_create(2, 3, 0)
    CN = spmv.csr_wrap_device(8, 9, 4, FAKE_RP, FAKE_CI, FAKE_VA)            # a pattern of the product's shape
    before = _untouched(C)
    lib = spmv.lib()
    for entry, call in (("spgemm_csr", spmv.spgemm_csr), ("spgemm_csr_numeric", spmv.spgemm_csr_numeric)):
        raw = getattr(lib, "spmv_c_" + entry)
        target = C if entry == "spgemm_csr" else CN
        # 1. nulls
        out = spmv.SpGEMMResult(error_code=7, nnz=9)
        assert raw(None, A, B, ctypes.byref(out)) == E.INVALID_ARGUMENT
        assert out.error_code == E.INVALID_ARGUMENT and out.nnz == 0
        assert raw(C, None, B, None) == E.INVALID_ARGUMENT                   # the result may be NULL
        assert raw(C, A, None, None) == E.INVALID_ARGUMENT
        # 2. C aliases A or B, before the dimensions
        assert call(A, A, W).error_code == E.INVALID_ARGUMENT
        assert call(W, A, W).error_code == E.INVALID_ARGUMENT
        # 3. the inner dimension, before the arrays
        assert call(target, A, W).error_code == E.INVALID_DIMENSION
        assert call(target, H, W).error_code == E.INVALID_DIMENSION
        # 4. missing device arrays
        for bad in (H, NC):
            assert call(target, A, bad).error_code == E.INVALID_FORMAT, entry
        A0 = spmv.csr_wrap_device(8, 0, 0, FAKE_RP, None, None)
        assert call(target, A0, Z).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(A0)
    # spgemm_csr_numeric: C's own shape and arrays, after the inner dimension
    assert spmv.spgemm_csr_numeric(C, A, B).error_code == E.INVALID_DIMENSION      # C is 2 x 3, not 8 x 9
    C89 = spmv.csr_create(8, 9, 4)
    assert spmv.spgemm_csr_numeric(C89, A, B).error_code == E.INVALID_FORMAT       # C has no device arrays
    spmv.csr_destroy(C89)
    assert _untouched(C) == before and not C.contents.owns_device_memory
    for M in (A, B, W, H, NC, Z, C, CN):
        spmv.csr_destroy(M)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_spgemm_cpu_csr_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-spgemm builds tests/cpp/bin/spgemm_host_sanitized (csrc/spgemm_host.cpp and
    tests/cpp/spgemm_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-spgemm"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "spgemm_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
