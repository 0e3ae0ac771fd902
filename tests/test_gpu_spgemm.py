"""spgemm_csr / spgemm_csr_numeric (include/spmv/spgemm.h) on the GPU, at zero tolerance against spgemm_cpu_csr on the
downloaded host arrays: row pointers, columns and value bits (NaNs by position).  The shapes come from
spgemm_class_capacity: every accumulator class at its edges, natural and forced; tables whose every insertion
collides and wraps; a row whose symbolic and numeric classes differ; every lane count; the dense class with a column
count that is no multiple of 32, one scratch slice and rows that must find it clean; a matrix that covers all classes
at once; special values; A^T A; the values-only pass and its pattern check; device validation; array views; empty
results; and a C++ caller."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import spgemm_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

INT_MAX = 2**31 - 1


def _caps(gpu):
    caps, cls = [], 1
    while gpu.spgemm_class_capacity(cls) != INT_MAX:
        caps.append(gpu.spgemm_class_capacity(cls))
        cls += 1
    return caps                                   # caps[c - 1] = capacity of LDS class c; the dense class is len + 1


def _class_of(caps, distinct, forced=0):
    if distinct == 0:
        return 0
    natural = next((c + 1 for c, cap in enumerate(caps) if distinct <= cap), len(caps) + 1)
    return max(natural, forced)


def _upload(gpu, rows, cols, arrays):
    M = gpu.csr_from_arrays(rows, cols, *arrays)
    assert gpu.csr_to_gpu(M) == 0
    return M


def _download(gpu, C):
    assert gpu.csr_from_gpu(C) == 0
    return gpu.csr_host_arrays(C)


def _device_words(gpu, address, count):
    out = np.empty(count, np.uint32)
    if count:
        assert gpu.lib().spmv_c_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(address), 4 * count) == 0
    return out


def _host(gpu, A, B):
    C = gpu.csr_create(0, 0, 0)
    assert gpu.spgemm_cpu_csr(C, A, B) == 0
    want = gpu.csr_host_arrays(C)
    gpu.csr_destroy(C)
    return want


def _product(gpu, A, B, want=None, what=""):
    """spgemm_csr(A, B) against the host product: (result, C's arrays)."""
    want = _host(gpu, A, B) if want is None else want
    C = gpu.csr_create(3, 3, 2)
    res = gpu.spgemm_csr(C, A, B)
    assert res.error_code == 0, (what, res.error_code)
    m = C.contents
    assert (m.num_rows, m.num_cols) == (A.contents.num_rows, B.contents.num_cols) and m.owns_device_memory
    got = _download(gpu, C)
    gpu.csr_destroy(C)
    sc.assert_same(got, want, what)
    assert res.nnz == want[1].size and res.max_row_nnz == (int(np.diff(want[0]).max()) if want[0].size > 1 else 0)
    assert sum(res.symbolic_rows) == sum(res.numeric_rows) == A.contents.num_rows
    return res, got


def _pair(gpu, m, k, n, a, b):
    return _upload(gpu, m, k, a), _upload(gpu, k, n, b)


def _rows_with_distinct(rng, n, counts, must_have=()):
    """A (one row per count) and B such that row i of A*B has exactly counts[i] distinct columns out of n, through
    two B rows that overlap (products = 1.5 x distinct, so the symbolic key is larger than the numeric one)."""
    a_rows, b_rows = [], []
    for d in counts:
        need = np.asarray(list(must_have)[:d], np.int64)
        pool = np.setdiff1d(rng.choice(n, size=d + need.size, replace=False), need)[:d - need.size]
        cols = np.sort(np.concatenate([pool, need]))
        assert cols.size == d and np.unique(cols).size == d
        first = len(b_rows)
        b_rows.append([(int(c), float(v)) for c, v in zip(cols, rng.uniform(-2, 2, d))])
        half = cols[::2]
        b_rows.append([(int(c), float(v)) for c, v in zip(half, rng.uniform(-2, 2, half.size))])
        a_rows.append([(first, float(rng.uniform(-2, 2))), (first + 1, float(rng.uniform(-2, 2)))])
    return sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows), len(b_rows)


# ---- classes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [1, 2, 3, 4])
def test_every_lds_class_at_its_capacity_natural_and_forced(gpu, monkeypatch, cls):
    caps = _caps(gpu)
    cap = caps[cls - 1]
    n = 3_000_001                                  # a table cannot be mistaken for a dense array
    counts = [3, cap - 1, cap, cap + 1]
    rng = np.random.default_rng(100 + cls)
    a, b, k = _rows_with_distinct(rng, n, counts, must_have=(0, n - 1))
    A, B = _pair(gpu, len(counts), k, n, a, b)
    want = _host(gpu, A, B)
    assert np.diff(want[0]).tolist() == counts
    try:
        for forced in (0, cls):
            if forced:
                monkeypatch.setenv("SPMV_DEBUG", f"spgemm_class={forced}")
            res, _ = _product(gpu, A, B, want, f"class {cls} forced {forced}")
            expect = [0] * 8
            for d in counts:
                expect[_class_of(caps, d, forced)] += 1
            assert list(res.numeric_rows) == expect, (forced, list(res.numeric_rows))
            assert res.numeric_rows[cls] >= 2 and res.numeric_rows[cls + 1] == 1     # cap ran in cls, cap + 1 in cls + 1
            expect = [0] * 8
            for d in counts:
                expect[_class_of(caps, min(d + (d + 1) // 2, n), forced)] += 1       # products = d + ceil(d / 2)
            assert list(res.symbolic_rows) == expect
            assert res.products == sum(d + (d + 1) // 2 for d in counts)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


@pytest.mark.parametrize("which", ["smallest", "largest"])
def test_every_insertion_collides_and_the_probe_wraps(gpu, which):
    caps = _caps(gpu)
    cls = 1 if which == "smallest" else len(caps)
    slots = 2 * caps[cls - 1]
    # the smallest class full to its capacity; the largest just past the class below it (every key still collides)
    count = caps[0] if which == "smallest" else caps[-2] + caps[-1] // 4
    cols = np.arange(count, dtype=np.int64) * slots + slots - 1
    n = int(cols[-1]) + 1
    rng = np.random.default_rng(7)
    b_rows = [[(int(c), float(v)) for c, v in zip(cols, rng.uniform(-2, 2, count))],
              [(int(c), float(v)) for c, v in zip(cols[1::3], rng.uniform(-2, 2, cols[1::3].size))]]
    a = sc.csr_from_rows([[(0, 1.5), (1, -0.75), (0, 0.5)]])
    A, B = _pair(gpu, 1, 2, n, a, sc.csr_from_rows(b_rows))
    res, got = _product(gpu, A, B, None, which)
    assert res.numeric_rows[cls] == 1 and got[1].size == count
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


def test_symbolic_and_numeric_pass_take_different_classes(gpu):
    rng = np.random.default_rng(8)
    b_rows = [[(5, float(rng.uniform(-1, 1))), (77, float(rng.uniform(-1, 1))), (4000, float(rng.uniform(-1, 1)))]
              for _ in range(600)]
    a = sc.csr_from_rows([[(k, float(rng.uniform(-1, 1))) for k in range(600)]])
    A, B = _pair(gpu, 1, 600, 5000, a, sc.csr_from_rows(b_rows))
    res, got = _product(gpu, A, B)
    caps = _caps(gpu)
    assert res.products == 1800 and res.max_row_products == 1800 and got[1].tolist() == [5, 77, 4000]
    sym, num = list(res.symbolic_rows).index(1), list(res.numeric_rows).index(1)
    assert sym == _class_of(caps, 1800) and num == _class_of(caps, 3) and sym != num
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


# ---- lanes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_every_lane_count(gpu, monkeypatch, lanes):
    rng = np.random.default_rng(lanes)
    lengths = [0, 1, lanes - 1, lanes, lanes + 1, 2 * lanes + 1]
    n = 2 * 64 + 3
    b_rows = [[(int(c) + (r % 2), float(v)) for c, v in zip(range(length), rng.uniform(-3, 3, length))]
              for r, length in enumerate(lengths)]
    a_rows = []
    for start in range(len(lengths)):
        for entries in (1, 2, 5):
            a_rows.append([((start + j) % len(lengths), float(rng.uniform(-3, 3))) for j in range(entries)])
    A, B = _pair(gpu, len(a_rows), len(lengths), n, sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows))
    monkeypatch.setenv("SPMV_DEBUG", f"spgemm_lanes={lanes}")
    try:
        res, _ = _product(gpu, A, B, None, f"lanes {lanes}")
        assert res.lanes == lanes
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- the dense class -----------------------------------------------------------------------------------------
def test_dense_class_edges_scratch_reuse_and_natural_choice(gpu, monkeypatch):
    caps = _caps(gpu)
    dense = len(caps) + 1
    n = 1_000_003                                  # no multiple of 32 or 64
    rng = np.random.default_rng(9)
    d = caps[-1] + 1
    big = np.sort(np.concatenate([[0, n - 1], np.setdiff1d(rng.choice(n, size=d + 2, replace=False), [0, n - 1])[:d - 2]]))
    assert big[0] == 0 and big[-1] == n - 1
    shared = big[::3]
    others = np.setdiff1d(np.arange(31, 31 + 64 * 50, 50), big)
    val = lambda c: [(int(x), float(v)) for x, v in zip(c, rng.uniform(-2, 2, len(c)))]
    b_rows = [val(big), val(np.union1d(shared, [1, n - 2])), val(others), val([0, n - 1])]
    a_rows = [[(0, 1.25), (1, -0.5)],              # more than the largest table holds: dense by itself
              [(1, 2.0), (3, 0.75), (1, -1.0)],    # shares columns with the row before it
              [(2, 3.0)],                          # touches none of them
              [(3, -4.0)]]                         # column 0 and column n - 1 only
    A, B = _pair(gpu, 4, 4, n, sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows))
    want = _host(gpu, A, B)
    assert np.diff(want[0])[0] >= caps[-1] + 1 and want[1][want[0][3]:].tolist() == [0, n - 1]
    try:
        res, _ = _product(gpu, A, B, want, "natural")
        assert res.numeric_rows[dense] == 1 and res.symbolic_rows[dense] == 1
        for setting in (f"spgemm_class={dense},spgemm_dense_groups=1", f"spgemm_class={dense}"):
            monkeypatch.setenv("SPMV_DEBUG", setting)
            res, _ = _product(gpu, A, B, want, setting)
            assert res.numeric_rows[dense] == 4 and res.symbolic_rows[dense] == 4
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- all classes at once -------------------------------------------------------------------------------------
class Mixed:
    """300 rows whose lengths cover every class at once; A unsorted with duplicates."""

    def __init__(self, gpu):
        rng = np.random.default_rng(11)
        caps = _caps(gpu)
        self.n, self.k, self.m = 40_000, 2000, 300
        long_lengths = [caps[0] * 5, caps[1] - 1, caps[1] * 6, caps[2] + 70, caps[2] * 3, caps[3] - 5, caps[3] + 1,
                        caps[3] + 800]
        lengths = [int(x) for x in rng.integers(0, 13, size=self.k - len(long_lengths))] + long_lengths
        b_rows = []
        for length in lengths:
            cols = np.sort(rng.choice(self.n, size=length, replace=False))
            b_rows.append(list(zip(cols.tolist(), rng.uniform(-2, 2, length).astype(np.float32).tolist())))
        a_rows = []
        short = self.k - len(long_lengths)
        for i in range(self.m):
            picks = rng.integers(0, short, size=int(rng.integers(0, 7))).tolist()
            if i >= self.m - 2 * len(long_lengths):
                picks.append(short + (i % len(long_lengths)))
            if picks:
                picks += [picks[int(rng.integers(0, len(picks)))]]              # a repeated entry
            picks = rng.permutation(picks).tolist()
            a_rows.append([(int(p), float(rng.uniform(-2, 2))) for p in picks])
        self.a, self.b = sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows)
        self.A, self.B = _pair(gpu, self.m, self.k, self.n, self.a, self.b)
        self.want = _host(gpu, self.A, self.B)


@pytest.fixture(scope="module")
def mixed(gpu):
    return Mixed(gpu)


def test_mixed_matrix_covers_every_class_and_is_reproducible(gpu, mixed):
    res, first = _product(gpu, mixed.A, mixed.B, mixed.want, "mixed")
    dense = len(_caps(gpu)) + 1
    assert all(res.numeric_rows[c] > 0 for c in range(dense + 1)), list(res.numeric_rows)
    assert all(res.symbolic_rows[c] > 0 for c in range(1, dense + 1)), list(res.symbolic_rows)
    _, second = _product(gpu, mixed.A, mixed.B, mixed.want, "mixed again")
    for x, y in zip(first, second):
        assert x.tobytes() == y.tobytes()


def test_numeric_pass_alone_refills_every_class(gpu, mixed):
    C = gpu.csr_create(0, 0, 0)
    assert gpu.spgemm_csr(C, mixed.A, mixed.B).error_code == 0
    m = C.contents
    structure = (_device_words(gpu, m.d_row_ptrs, m.num_rows + 1), _device_words(gpu, m.d_col_indices, m.nnz))
    new_vals = (mixed.a[2] * np.float32(0.5) + np.float32(0.125)).astype(np.float32)
    A2 = _upload(gpu, mixed.m, mixed.k, (mixed.a[0], mixed.a[1], new_vals))
    want = _host(gpu, A2, mixed.B)
    # overwrite A's device values in place
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(mixed.A.contents.d_values),
                                       new_vals.ctypes.data_as(ctypes.c_void_p), new_vals.nbytes) == 0
    try:
        res = gpu.spgemm_csr_numeric(C, mixed.A, mixed.B)
        assert res.error_code == 0 and res.nnz == m.nnz
        dense = len(_caps(gpu)) + 1
        assert all(res.numeric_rows[c] > 0 for c in range(dense + 1)) and sum(res.symbolic_rows) == 0
        sc.assert_same(_download(gpu, C), want, "numeric alone")
        after = (_device_words(gpu, m.d_row_ptrs, m.num_rows + 1), _device_words(gpu, m.d_col_indices, m.nnz))
        assert structure[0].tobytes() == after[0].tobytes() and structure[1].tobytes() == after[1].tobytes()
    finally:
        assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(mixed.A.contents.d_values),
                                           mixed.a[2].ctypes.data_as(ctypes.c_void_p), mixed.a[2].nbytes) == 0
        gpu.csr_destroy(A2)
        gpu.csr_destroy(C)


def test_numeric_pass_alone_rejects_a_pattern_that_is_not_the_products(gpu):
    E = gpu.SpMVError
    rng = np.random.default_rng(12)
    a, b = sc.random_csr(rng, 37, 23, 0.3), sc.random_csr(rng, 23, 41, 0.3)
    A, B = _pair(gpu, 37, 23, 41, a, b)
    C = gpu.csr_create(0, 0, 0)
    assert gpu.spgemm_csr(C, A, B).error_code == 0
    rp, ci, _ = _download(gpu, C)
    assert gpu.spgemm_csr_numeric(C, A, B).error_code == 0
    put = lambda address, array: gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(address),
                                                             array.ctypes.data_as(ctypes.c_void_p), array.nbytes)
    # one column changed to one the row does not produce
    row = next(i for i in range(37) if 0 < rp[i + 1] - rp[i] < 41)
    absent = int(np.setdiff1d(np.arange(41), ci[rp[row]:rp[row + 1]])[0])
    changed = ci.copy()
    changed[rp[row]] = absent
    assert put(C.contents.d_col_indices, changed) == 0
    assert gpu.spgemm_csr_numeric(C, A, B).error_code == E.INVALID_FORMAT
    assert put(C.contents.d_col_indices, ci) == 0
    assert gpu.spgemm_csr_numeric(C, A, B).error_code == 0
    # one row shortened (the next one takes its last entry: the row pointers stay well formed)
    row = next(i for i in range(36) if rp[i + 1] - rp[i] > 1)
    shorter = rp.copy()
    shorter[row + 1] -= 1
    assert put(C.contents.d_row_ptrs, shorter) == 0
    assert gpu.spgemm_csr_numeric(C, A, B).error_code == E.INVALID_FORMAT
    assert put(C.contents.d_row_ptrs, rp) == 0
    assert gpu.spgemm_csr_numeric(C, A, B).error_code == 0
    for M in (A, B, C):
        gpu.csr_destroy(M)


# ---- values --------------------------------------------------------------------------------------------------
def test_special_values_and_cancelled_entries(gpu):
    inf, nan = np.inf, np.nan
    a_rows = [[(0, -0.0)], [(0, 1.0), (1, -1.0)], [(1, inf), (2, -inf), (0, 2.0)], [(2, nan), (3, 0.0)],
              [(3, inf)], [(0, -0.0), (1, 0.0), (2, 1e38)]]
    b_rows = [[(0, 1.0), (3, -0.0)], [(0, 1.0), (2, inf)], [(1, 1e38), (2, inf), (3, 0.0)], [(0, nan), (1, 0.0), (3, -inf)]]
    A, B = _pair(gpu, 6, 4, 4, sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows))
    res, (rp, ci, va) = _product(gpu, A, B)
    assert sc.bits(va[rp[0]:rp[1]]).tolist() == [0, 0]                 # +0.0 + -0.0 = +0.0, and -0.0 * -0.0 = +0.0
    assert ci[rp[1]:rp[2]].tolist() == [0, 2, 3] and sc.bits(va[rp[1]:rp[1] + 1]).tolist() == [0]    # cancelled, kept
    assert np.isnan(va).any() and np.isinf(va).any()
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


def test_at_a_through_the_device_transpose(gpu):
    rng = np.random.default_rng(13)
    rows, cols = 200, 50
    rp, ci, va = sc.random_csr(rng, rows, cols, 0.12)
    A = _upload(gpu, rows, cols, (rp, ci, va))
    AT = gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(AT, A) == 0
    order = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=cols))]).astype(np.int32)
    HT = gpu.csr_from_arrays(cols, rows, t_rp, row_of[order], va[order])
    want = _host(gpu, HT, A)
    res, (c_rp, c_ci, c_va) = _product(gpu, AT, A, want, "A^T A")
    dense = np.full((cols, cols), 0xFFFFFFFF, np.uint64)               # value bits; all ones = not stored
    dense[np.repeat(np.arange(cols), np.diff(c_rp)), c_ci] = sc.bits(c_va)
    np.testing.assert_array_equal(dense, dense.T)
    assert (dense != 0xFFFFFFFF).sum() == c_ci.size > cols
    for M in (A, AT, HT):
        gpu.csr_destroy(M)


# ---- validation, views, empty results ------------------------------------------------------------------------
def test_device_validation_leaves_c_untouched(gpu):
    E = gpu.SpMVError
    f32 = lambda v: np.asarray(v, np.float32)
    good_a = ([0, 2, 3], [0, 2, 1], f32([1, 2, 3]))
    good_b = ([0, 1, 3, 4], [0, 1, 3, 2], f32([1, 2, 3, 4]))
    bad = {
        "A's column equals B.num_rows": (([0, 2, 3], [0, 3, 1], f32([1, 2, 3])), good_b),
        "A's column negative": (([0, 2, 3], [0, -1, 1], f32([1, 2, 3])), good_b),
        "A's row pointers decrease": (([0, 3, 2], [0, 2, 1], f32([1, 2, 3])), good_b),
        "B with an equal adjacent pair": (good_a, ([0, 1, 3, 4], [0, 1, 1, 2], f32([1, 2, 3, 4]))),
        "B with a descending pair": (good_a, ([0, 1, 3, 4], [0, 3, 1, 2], f32([1, 2, 3, 4]))),
        "B's column out of range": (good_a, ([0, 1, 3, 4], [0, 1, 4, 2], f32([1, 2, 3, 4]))),
        "B's row pointers do not end at nnz": (good_a, ([0, 1, 3, 3], [0, 1, 3, 2], f32([1, 2, 3, 4]))),
    }
    C = gpu.csr_create(2, 3, 1)
    field = lambda: (C.contents.num_rows, C.contents.num_cols, C.contents.nnz, bool(C.contents.owns_device_memory),
                     C.contents.d_row_ptrs, C.contents.d_col_indices, C.contents.d_values)
    before = field()
    for name, (a, b) in bad.items():
        A, B = _pair(gpu, 2, 3, 4, a, b)
        assert gpu.spgemm_csr(C, A, B).error_code == E.INVALID_FORMAT, name
        assert field() == before, name
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)
    A, B = _pair(gpu, 2, 3, 4, good_a, good_b)              # a row of B may start below where the row before it ended
    res, _ = _product(gpu, A, B)
    assert res.error_code == 0
    for M in (A, B, C):
        gpu.csr_destroy(M)


@pytest.mark.parametrize("offsets", [(1, 2, 3), (3, 1, 2)])
def test_inputs_that_are_views_into_larger_buffers(gpu, offsets):
    rng = np.random.default_rng(14)
    a = sc.random_csr(rng, 61, 43, 0.2, sort=False, duplicates=True)
    b = sc.random_csr(rng, 43, 300, 0.15)
    HA, HB = gpu.csr_from_arrays(61, 43, *a), gpu.csr_from_arrays(43, 300, *b)
    want = _host(gpu, HA, HB)
    with av.Views(gpu) as V:
        A, _ = V.csr(61, 43, *a, offsets)
        B, _ = V.csr(43, 300, *b, offsets[::-1])
        C = gpu.csr_create(0, 0, 0)
        assert gpu.spgemm_csr(C, A, B).error_code == 0
        V.check_guards(("spgemm_csr", offsets))
        sc.assert_same(_download(gpu, C), want, "views")
        assert gpu.spgemm_csr_numeric(C, A, B).error_code == 0
        V.check_guards(("spgemm_csr_numeric", offsets))
        sc.assert_same(_download(gpu, C), want, "views, numeric")
        gpu.csr_destroy(C)
    gpu.csr_destroy(HA)
    gpu.csr_destroy(HB)


def test_empty_results(gpu):
    empty = lambda r: (np.zeros(r + 1, np.int32), np.empty(0, np.int32), np.empty(0, np.float32))
    b_rows = [[(0, 2.0), (4, -1.0)], [], [(1, 0.75)], []]
    cases = {
        "m = 0": (0, 4, 6, empty(0), sc.csr_from_rows(b_rows)),
        "n = 0": (5, 4, 0, sc.csr_from_rows([[(1, 1.0)], [], [(3, 2.0)], [], []]), empty(4)),
        "nnz(A) = 0": (5, 4, 6, empty(5), sc.csr_from_rows(b_rows)),
        "only empty rows of B": (3, 4, 6, sc.csr_from_rows([[(1, 1.0), (3, 2.0)], [], [(3, -1.0)]]),
                                 sc.csr_from_rows(b_rows)),
    }
    for name, (m, k, n, a, b) in cases.items():
        A, B = _pair(gpu, m, k, n, a, b)
        res, (rp, ci, va) = _product(gpu, A, B, None, name)
        assert res.nnz == 0 and ci.size == 0 and rp.tolist() == [0] * (m + 1), name
        assert res.numeric_rows[0] == m and res.symbolic_rows[0] == m
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- a C++ caller --------------------------------------------------------------------------------------------
def test_cpp_spgemm_smoke(gpu, tmp_path):
    """tests/cpp/spgemm_smoke.cpp through spmv/spgemm.h, csr_matrix.h and CudaBuffer, compiled here with build()'s
    g++ line."""
    exe = str(tmp_path / "spgemm_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "spgemm_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
