"""csr_add / csr_add_numeric / csr_add_cpu, csr_scale, csr_diagonal and csr_diag_matrix (include/spmv/csr_ops.h) on the
host side (no GPU): the exported names and the result layout; csr_add_cpu against a plain restatement of the
three-case rule, bit for bit, and against int64 arithmetic on small-integer matrices; cancellation, 0 * Inf, -0.0 and
A + A; every check that needs no device, in the stated order, with fake device addresses that must never be
dereferenced; the host twins of scaling and the diagonal against their numpy forms; and the sanitized caller."""
import ctypes
import os
import re
import subprocess

import numpy as np

import csr_ops_cases as oc
from conftest import ROOT

NAMES = ("csr_add", "csr_add_numeric", "csr_add_cpu", "csr_scale_gpu", "csr_scale_cpu", "csr_diagonal_gpu",
         "csr_diagonal_cpu", "csr_diag_matrix_gpu", "csr_diag_matrix_cpu")

# fake, never-dereferenced device addresses: every call below must return before it touches them
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


# ---- names and layouts ---------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)                     # what test_host_library.py checks
    cxx = open(os.path.join(ROOT, "include", "spmv", "csr_ops.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared and "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert "spmv_c_csr_add_result" in header


def test_result_layout_and_defaults(spmv):
    R = spmv.CsrAddResult
    assert ctypes.sizeof(R) == 32
    names = ["error_code", "nnz", "common", "max_row_nnz", "lanes", "launches", "symbolic_ms", "numeric_ms"]
    assert [f for f, _ in R._fields_] == names
    assert [getattr(R, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 28]
    # what a rejected call leaves: the defaults of the C++ constructor and the code
    out = R(error_code=7, nnz=9, common=3, max_row_nnz=4, lanes=5, launches=6, symbolic_ms=1.0, numeric_ms=2.0)
    assert spmv.lib().spmv_c_csr_add(None, 1.0, None, 1.0, None, ctypes.byref(out)) == spmv.SpMVError.INVALID_ARGUMENT
    assert [getattr(out, f) for f in names] == [spmv.SpMVError.INVALID_ARGUMENT, 0, 0, 0, 0, 0, 0.0, 0.0]


# ---- the arithmetic ------------------------------------------------------------------------------------------
def test_cpu_sum_equals_the_restated_rule_bit_for_bit(spmv):
    rng = np.random.default_rng(30)
    shapes = [(37, 23), (23, 41), (1, 64), (50, 1), (19, 19)]
    checked = 0
    for density_a in (0.0, 0.05, 0.2, 0.5):
        for density_b in (0.0, 0.1, 0.5):
            m, n = shapes[checked % len(shapes)]
            a, b = oc.random_csr(rng, m, n, density_a), oc.random_csr(rng, m, n, density_b)
            for alpha, beta in ((1, 1), (1, -1), (0, 1), (-1, 0), (0.5, 0.5), (0, 0),
                                tuple(rng.uniform(-3, 3, 2).astype(np.float32))):
                status, got = oc.host_sum(spmv, m, n, alpha, a, beta, b)
                assert status == 0
                oc.assert_same(got, oc.add_loop(m, alpha, a, beta, b), (m, n, density_a, density_b, alpha, beta))
                assert got[0].size == m + 1
            checked += 1
    # special values on both sides
    a = oc.with_specials(rng, oc.random_csr(rng, 40, 30, 0.4), 0.3)
    b = oc.with_specials(rng, oc.random_csr(rng, 40, 30, 0.4), 0.3)
    for alpha, beta in ((1, 1), (0, 2), (-0.0, np.inf), (1e-30, 1e30)):
        status, got = oc.host_sum(spmv, 40, 30, alpha, a, beta, b)
        assert status == 0
        oc.assert_same(got, oc.add_loop(40, alpha, a, beta, b), ("specials", alpha, beta))
    assert np.isnan(got[2]).any()
    # the empty shapes
    for m, n in ((0, 5), (5, 0), (0, 0), (4, 6)):
        status, got = oc.host_sum(spmv, m, n, 2.0, oc.empty(m), 3.0, oc.empty(m))
        assert status == 0 and got[0].tolist() == [0] * (m + 1) and got[1].size == 0


def test_cpu_sum_equals_int64_arithmetic_on_small_integers(spmv):
    rng = np.random.default_rng(31)
    m, n = 60, 45
    da = rng.integers(-8, 9, size=(m, n)) * (rng.random((m, n)) < 0.3)
    db = rng.integers(-8, 9, size=(m, n)) * (rng.random((m, n)) < 0.3)
    to_csr = lambda d: oc.csr_from_rows([[(int(c), float(d[i, c])) for c in np.flatnonzero(d[i])] for i in range(m)])
    for alpha, beta in ((1, 1), (2, -4), (-0.5, 0.25), (8, 0.125), (1, -1)):  # powers of two: every step is exact
        status, (rp, ci, va) = oc.host_sum(spmv, m, n, alpha, to_csr(da), beta, to_csr(db))
        assert status == 0
        exact8 = (int(alpha * 8) * da.astype(np.int64) + int(beta * 8) * db.astype(np.int64))      # 8 C, in integers
        pattern = (da != 0) | (db != 0)
        for i in range(m):
            cols = ci[rp[i]:rp[i + 1]]
            np.testing.assert_array_equal(cols, np.flatnonzero(pattern[i]))
            np.testing.assert_array_equal((va[rp[i]:rp[i + 1]].astype(np.float64) * 8).astype(np.int64), exact8[i, cols])
    assert (va == 0).any()                                                   # cancelled entries are stored


def test_cancellation_zero_times_inf_and_negative_zero(spmv):
    a = oc.csr_from_rows([[(0, 1.5), (3, -2.0)], [(1, np.inf), (2, 4.0)], [(2, -0.0)], [(0, 0.0)]])
    # A + (-1) A: the full pattern, every value +0.0f (Inf - Inf is a NaN, in place)
    status, (rp, ci, va) = oc.host_sum(spmv, 4, 4, 1.0, a, -1.0, a)
    assert status == 0 and rp.tolist() == a[0].tolist() and ci.tolist() == a[1].tolist()
    assert np.isnan(va[2]) and oc.bits(np.delete(va, 2)).tolist() == [0] * 5
    # alpha = 0 removes nothing and 0 * Inf is the NaN the rule says
    status, (rp, ci, va) = oc.host_sum(spmv, 4, 4, 0.0, a, 1.0, oc.csr_from_rows([[], [(3, 7.0)], [], []]))
    assert status == 0 and rp.tolist() == [0, 2, 5, 6, 7] and ci.tolist() == [0, 3, 1, 2, 3, 2, 0]
    assert np.isnan(va[2]) and va[4] == 7.0
    assert oc.bits(va[[0, 1, 3, 5, 6]]).tolist() == oc.bits([0.0, -0.0, 0.0, -0.0, 0.0]).tolist()
    # -0.0f survives on a one-sided entry, from either side
    status, (rp, ci, va) = oc.host_sum(spmv, 4, 4, 1.0, a, 1.0, oc.csr_from_rows([[], [], [(0, -0.0)], []]))
    assert status == 0 and ci[rp[2]:rp[3]].tolist() == [0, 2]
    assert oc.bits(va[rp[2]:rp[3]]).tolist() == oc.bits([-0.0, -0.0]).tolist()
    # an explicit zero is an entry
    assert ci[rp[3]:rp[4]].tolist() == [0] and oc.bits(va[rp[3]:rp[4]]).tolist() == [0]


def test_a_may_be_b(spmv):
    rng = np.random.default_rng(32)
    a = oc.random_csr(rng, 31, 19, 0.3)
    A = spmv.csr_from_arrays(31, 19, *a)
    C = spmv.csr_create(0, 0, 0)
    assert spmv.csr_add_cpu(C, 1.0, A, 1.0, A) == 0
    rp, ci, va = spmv.csr_host_arrays(C)
    oc.assert_same((rp, ci, va), (a[0], a[1], a[2] * np.float32(2.0)), "A + A")
    spmv.csr_destroy(A)
    spmv.csr_destroy(C)


# ---- rejections ----------------------------------------------------------------------------------------------
def _untouched(C):
    m = C.contents
    return (m.num_rows, m.num_cols, m.nnz, bool(m.owns_device_memory), m.d_row_ptrs, m.d_col_indices, m.d_values)


def test_cpu_checks_in_the_stated_order_with_c_untouched(spmv):
    E = spmv.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    A = spmv.csr_from_arrays(3, 4, [0, 1, 3, 4], [0, 1, 3, 2], f32([1, 2, 3, 4]))
    WR = spmv.csr_from_arrays(2, 4, [0, 1, 2], [0, 1], f32([1, 1]))          # other rows
    WC = spmv.csr_from_arrays(3, 5, [0, 1, 2, 2], [0, 4], f32([1, 1]))       # other columns
    C = spmv.csr_create(2, 3, 0)
    before = _untouched(C)
    lib = spmv.lib()
    assert lib.spmv_c_csr_add_cpu(None, 1.0, A, 1.0, A) == E.INVALID_ARGUMENT
    assert lib.spmv_c_csr_add_cpu(C, 1.0, None, 1.0, A) == E.INVALID_ARGUMENT
    assert lib.spmv_c_csr_add_cpu(C, 1.0, A, 1.0, None) == E.INVALID_ARGUMENT
    assert spmv.csr_add_cpu(A, 1.0, A, 1.0, WR) == E.INVALID_ARGUMENT        # alias before the dimension check
    assert spmv.csr_add_cpu(WR, 1.0, A, 1.0, WR) == E.INVALID_ARGUMENT
    assert spmv.csr_add_cpu(C, 1.0, A, 1.0, WR) == E.INVALID_DIMENSION
    assert spmv.csr_add_cpu(C, 1.0, WC, 1.0, A) == E.INVALID_DIMENSION
    bad = {
        "two equal adjacent columns": ([0, 1, 3, 4], [0, 1, 1, 2]),
        "one descending pair": ([0, 1, 3, 4], [0, 3, 1, 2]),
        "column out of range": ([0, 1, 3, 4], [0, 1, 4, 2]),
        "negative column": ([0, 1, 3, 4], [0, -1, 3, 2]),
        "row_ptrs decrease": ([0, 3, 1, 4], [0, 1, 3, 2]),
        "row_ptrs do not start at 0": ([1, 1, 3, 4], [0, 1, 3, 2]),
        "row_ptrs do not end at nnz": ([0, 1, 3, 3], [0, 1, 3, 2]),
    }
    for name, (rp, ci) in bad.items():
        X = spmv.csr_from_arrays(3, 4, rp, ci, f32([1, 2, 3, 4]))
        assert spmv.csr_add_cpu(C, 1.0, A, 1.0, X) == E.INVALID_FORMAT, name
        assert spmv.csr_add_cpu(C, 1.0, X, 1.0, A) == E.INVALID_FORMAT, name
        spmv.csr_destroy(X)
    assert _untouched(C) == before
    assert spmv.csr_add_cpu(C, 1.0, A, 1.0, A) == 0 and C.contents.num_cols == 4 and C.contents.owns_host_memory
    for M in (A, WR, WC, C):
        spmv.csr_destroy(M)


def test_device_entry_checks_in_the_stated_order_before_any_device_work(spmv):
    E = spmv.SpMVError
    A = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    B = spmv.csr_wrap_device(8, 6, 12, FAKE_RP, FAKE_CI, FAKE_VA)
    WR = spmv.csr_wrap_device(5, 6, 12, FAKE_RP, FAKE_CI, FAKE_VA)           # other rows
    WC = spmv.csr_wrap_device(8, 9, 12, FAKE_RP, FAKE_CI, FAKE_VA)           # other columns
    H = spmv.csr_from_arrays(8, 6, np.arange(9, dtype=np.int32).clip(0, 6), np.arange(6, dtype=np.int32),
                             np.ones(6, np.float32))                         # host only
    HW = spmv.csr_from_arrays(5, 6, np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32), np.ones(5, np.float32))
    NC = spmv.csr_wrap_device(8, 6, 12, FAKE_RP, None, FAKE_VA)              # entries and no columns
    NV = spmv.csr_wrap_device(8, 6, 12, FAKE_RP, FAKE_CI, None)              # entries and no values
    C = spmv.csr_create(2, 3, 0)
    CN = spmv.csr_wrap_device(8, 6, 20, FAKE_RP, FAKE_CI, FAKE_VA)           # a pattern of the sum's shape
    before = _untouched(C)
    lib = spmv.lib()
    for entry, call in (("csr_add", spmv.csr_add), ("csr_add_numeric", spmv.csr_add_numeric)):
        raw = getattr(lib, "spmv_c_" + entry)
        target = C if entry == "csr_add" else CN
        # 1. nulls
        out = spmv.CsrAddResult(error_code=7, nnz=9)
        assert raw(None, 1.0, A, 1.0, B, ctypes.byref(out)) == E.INVALID_ARGUMENT
        assert out.error_code == E.INVALID_ARGUMENT and out.nnz == 0
        assert raw(C, 1.0, None, 1.0, B, None) == E.INVALID_ARGUMENT         # the result may be NULL
        assert raw(C, 1.0, A, 1.0, None, None) == E.INVALID_ARGUMENT
        # 2. C aliases A or B, before the dimensions
        assert call(A, 1.0, A, 1.0, WR).error_code == E.INVALID_ARGUMENT
        assert call(WR, 1.0, A, 1.0, WR).error_code == E.INVALID_ARGUMENT
        # 3. the dimensions, before the arrays
        assert call(target, 1.0, A, 1.0, WR).error_code == E.INVALID_DIMENSION
        assert call(target, 1.0, WC, 1.0, B).error_code == E.INVALID_DIMENSION
        assert call(target, 1.0, H, 1.0, HW).error_code == E.INVALID_DIMENSION
        # 4. missing device arrays
        for bad in (H, NC, NV):
            assert call(target, 1.0, A, 1.0, bad).error_code == E.INVALID_FORMAT, entry
            assert call(target, 1.0, bad, 1.0, B).error_code == E.INVALID_FORMAT, entry
        Z1 = spmv.csr_wrap_device(0, 6, 3, None, FAKE_CI, FAKE_VA)           # no rows cannot hold entries
        Z2 = spmv.csr_wrap_device(0, 6, 0, None, None, None)
        assert call(target, 1.0, Z1, 1.0, Z2).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(Z1)
        spmv.csr_destroy(Z2)
    # csr_add_numeric: C's own shape and arrays, after A's and B's
    assert spmv.csr_add_numeric(C, 1.0, A, 1.0, B).error_code == E.INVALID_DIMENSION         # C is 2 x 3, not 8 x 6
    assert spmv.csr_add_numeric(C, 1.0, A, 1.0, NC).error_code == E.INVALID_FORMAT           # B's arrays come first
    C86 = spmv.csr_create(8, 6, 4)
    assert spmv.csr_add_numeric(C86, 1.0, A, 1.0, B).error_code == E.INVALID_FORMAT          # C has no device arrays
    spmv.csr_destroy(C86)
    assert _untouched(C) == before and not C.contents.owns_device_memory
    for M in (A, B, WR, WC, H, HW, NC, NV, C, CN):
        spmv.csr_destroy(M)


def test_scale_diagonal_and_diag_matrix_checks_that_need_no_device(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    A = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    H = spmv.csr_create(8, 6, 4)
    NV = spmv.csr_wrap_device(8, 6, 12, FAKE_RP, FAKE_CI, None)
    r, c, out = 0x600000, 0x700000, 0x800000
    # csr_scale_gpu: null, arrays, then overlaps
    assert lib.spmv_c_csr_scale_gpu(None, r, c, out) == E.INVALID_ARGUMENT
    assert spmv.csr_scale_gpu(H, r, c, out) == E.INVALID_FORMAT
    assert spmv.csr_scale_gpu(NV, r, c, out) == E.INVALID_FORMAT
    assert spmv.csr_scale_gpu(H, r, c, r) == E.INVALID_FORMAT                # the arrays before the overlap
    assert spmv.csr_scale_gpu(A, r, c, FAKE_VA + 4) == E.INVALID_ARGUMENT    # the values, shifted by one
    assert spmv.csr_scale_gpu(A, r, c, FAKE_VA - 4 * 15) == E.INVALID_ARGUMENT
    assert spmv.csr_scale_gpu(A, r, c, r + 4 * 7) == E.INVALID_ARGUMENT      # the last row scale
    assert spmv.csr_scale_gpu(A, r, c, c - 4 * 15) == E.INVALID_ARGUMENT     # the first column scale
    assert spmv.csr_scale_gpu(A, FAKE_VA + 4 * 15, c, None) == E.INVALID_ARGUMENT            # in place over a scale
    assert spmv.csr_scale_gpu(A, r, FAKE_VA - 4 * 5, FAKE_VA) == E.INVALID_ARGUMENT
    # csr_diagonal_gpu
    assert lib.spmv_c_csr_diagonal_gpu(None, out) == E.INVALID_ARGUMENT
    assert spmv.csr_diagonal_gpu(A, None) == E.INVALID_ARGUMENT
    assert spmv.csr_diagonal_gpu(H, None) == E.INVALID_ARGUMENT              # the null before the arrays
    assert spmv.csr_diagonal_gpu(H, out) == E.INVALID_FORMAT
    # csr_diag_matrix_gpu
    assert lib.spmv_c_csr_diag_matrix_gpu(None, -1, out) == E.INVALID_ARGUMENT
    before = _untouched(H)
    assert spmv.csr_diag_matrix_gpu(H, -1, out) == E.INVALID_DIMENSION and _untouched(H) == before
    for M in (A, H, NV):
        spmv.csr_destroy(M)


# ---- the host twins ------------------------------------------------------------------------------------------
def _symmetric(rng, n, density):
    half = np.triu(rng.uniform(-2, 2, size=(n, n)) * (rng.random((n, n)) < density)).astype(np.float32)
    dense = half + half.T - np.diag(np.diag(half))
    rows = [[(int(c), float(dense[i, c])) for c in np.flatnonzero(dense[i])] for i in range(n)]
    return oc.csr_from_rows(rows)


def test_scale_cpu_against_numpy_and_the_bitwise_symmetry(spmv):
    rng = np.random.default_rng(33)
    m, n = 37, 29
    rp, ci, va = oc.with_specials(rng, oc.random_csr(rng, m, n, 0.3, sort=False, duplicates=True), 0.1)
    A = spmv.csr_from_arrays(m, n, rp, ci, va)
    r, c = rng.uniform(-2, 2, m).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)
    row_of = np.repeat(np.arange(m), np.diff(rp))
    with np.errstate(all="ignore"):
        forms = {(True, True): va * (r[row_of] * c[ci]), (True, False): va * r[row_of], (False, True): va * c[ci],
                 (False, False): va}
    for (use_r, use_c), want in forms.items():
        status, got = spmv.csr_scale_cpu(A, r if use_r else None, c if use_c else None)
        assert status == 0
        assert want.dtype == np.float32
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        keep = ~np.isnan(want)
        np.testing.assert_array_equal(oc.bits(got)[keep], oc.bits(want)[keep], err_msg=str((use_r, use_c)))
    spmv.csr_destroy(A)
    # r == c on a symmetric matrix: symmetric bit for bit, which a (a r_i) c_j evaluation is not
    n = 40
    rp, ci, va = _symmetric(rng, n, 0.3)
    S = spmv.csr_from_arrays(n, n, rp, ci, va)
    d = rng.uniform(0.1, 3, n).astype(np.float32)
    status, got = spmv.csr_scale_cpu(S, d, d)
    assert status == 0
    dense = np.full((n, n), 0xFFFFFFFF, np.uint64)
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = oc.bits(got)
    np.testing.assert_array_equal(dense, dense.T)
    row_of = np.repeat(np.arange(n), np.diff(rp))
    unfolded = np.full((n, n), 0xFFFFFFFF, np.uint64)
    unfolded[row_of, ci] = oc.bits((va * d[row_of]) * d[ci])
    assert (unfolded != unfolded.T).any()                                     # the property is the folding's
    # malformed structures and a null output
    E = spmv.SpMVError
    X = spmv.csr_from_arrays(2, 3, [0, 2, 3], [0, 3, 1], np.ones(3, np.float32))
    assert spmv.csr_scale_cpu(X, None, None)[0] == E.INVALID_FORMAT
    assert spmv.lib().spmv_c_csr_scale_cpu(S, None, None, None) == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_scale_cpu(None, None, None, None) == E.INVALID_ARGUMENT
    spmv.csr_destroy(X)
    spmv.csr_destroy(S)


def test_diagonal_cpu_and_diag_matrix_cpu(spmv):
    E = spmv.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    # row 0: two stored diagonal entries, summed in storage order; row 1: none; row 3 lies past the last column
    A = spmv.csr_from_arrays(4, 3, [0, 3, 4, 5, 6], [0, 2, 0, 0, 2, 1], f32([1e8, 9.0, 1.0, 4.0, -2.0, 6.0]))
    status, d = spmv.csr_diagonal_cpu(A)
    assert status == 0 and oc.bits(d).tolist() == oc.bits([np.float32(1e8) + np.float32(1.0), 0.0, -2.0, 0.0]).tolist()
    spmv.csr_destroy(A)
    rng = np.random.default_rng(34)
    n = 50
    rp, ci, va = oc.random_csr(rng, n, n, 0.2)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, d = spmv.csr_diagonal_cpu(A)
    dense = np.zeros((n, n), np.float32)
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    assert status == 0 and oc.bits(d).tolist() == oc.bits(np.diag(dense) + np.float32(0.0)).tolist()
    spmv.csr_destroy(A)
    # the diagonal matrix: zeros kept, the identity, the round trip, n = 0
    v = f32([2.0, 0.0, -3.5, np.inf, 1e-45])
    D = spmv.csr_create(2, 7, 1)
    assert spmv.csr_diag_matrix_cpu(D, 5, v) == 0
    rp, ci, va = spmv.csr_host_arrays(D)
    assert (D.contents.num_rows, D.contents.num_cols, D.contents.nnz) == (5, 5, 5)
    assert rp.tolist() == list(range(6)) and ci.tolist() == list(range(5)) and oc.bits(va).tolist() == oc.bits(v).tolist()
    status, back = spmv.csr_diagonal_cpu(D)
    assert status == 0 and oc.bits(back).tolist() == oc.bits(v).tolist()
    assert spmv.csr_diag_matrix_cpu(D, 3, None) == 0 and spmv.csr_host_arrays(D)[2].tolist() == [1.0, 1.0, 1.0]
    assert spmv.csr_diag_matrix_cpu(D, 0, None) == 0 and spmv.csr_host_arrays(D)[0].tolist() == [0]
    assert spmv.csr_diag_matrix_cpu(D, -2, None) == E.INVALID_DIMENSION and D.contents.num_rows == 0
    assert spmv.lib().spmv_c_csr_diag_matrix_cpu(None, 3, None) == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_diagonal_cpu(None, None) == E.INVALID_ARGUMENT
    spmv.csr_destroy(D)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_the_host_routines_are_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-csr-ops builds tests/cpp/bin/csr_ops_host_sanitized (csrc/csr_ops_host.cpp and
    tests/cpp/csr_ops_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-csr-ops"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "csr_ops_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
