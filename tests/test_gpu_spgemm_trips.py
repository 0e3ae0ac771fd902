"""spgemm_csr / spgemm_csr_numeric (csrc/spgemm.hip) past their grid caps and in every table geometry, and the structure
check of csr_transpose_gpu (csrc/transpose.hip) past its own, at zero tolerance.  The judge of every product is a numpy
or period reference (spgemm_cases.product_loop tiled, or int64 arithmetic proved exact); spgemm_cpu_csr is the second
witness.  tests/test_spgemm_trips_host.py proves what each case is named for.

A  every (class, lanes) geometry of spgemm_table_kernel: sub-wavefront workgroups, both passes, the values-only pass.
B  16 391 non-empty rows at 64 lanes: second trips of the table kernel in classes 1 .. 3, five trips in class 4, 65 trips
   of the dense kernel over 256 slices, with fewer map words than threads and with a second round of the write-out.
C  spgemm_products_kernel at 64 lanes per row of A, 16 389 rows: its second trip, with the longest row in it.
D  spgemm_classify_kernel's flag as the only one raised, from workgroup 4097.
E  spgemm_validate_kernel: one defect per call, seen by one work item at or above 524 288.
F  transpose_validate_kernel: the radix passes decided by single entries of its second trip.

The stride check, by reading.
* spgemm_table_kernel, `for base` (B).  Stopped after one trip, the SYMBOLIC pass leaves the rows of list positions
  16 384 .. 16 390 at the 0 that spgemm_build's memset put into c.row_ptrs (spgemm.hip:717): "row_ptrs" of assert_same
  and res.nnz fail.  The NUMERIC pass would leave their entries as the fresh allocation held them: "cols" / "value bits"
  fail unless the allocation held this very row, which the REFILL run excludes for the values: C's values are
  overwritten with a NaN sentinel first, so an unvisited row fails "NaN positions".  A stride too long skips rows: the
  same assertions.  A stride too short (gridDim.x for gridDim.x * tables) visits rows twice with equal results and
  changes no output: no test can see it here, it costs time only; in spgemm_products_kernel it counts rows twice and
  res.products fails (C).  Without the clear at the head of a trip the second trip finds the keys of another period row
  (the host test: rows one stride apart differ): the claim count is not the row's, so "row_ptrs" fails after SYMBOLIC,
  and NUMERIC / REFILL raise their flag: error_code == 0 fails.
* spgemm_dense_kernel, `for idx` (B, class 5): as above; a slice left dirty adds the bits of the row before to the
  count ("row_ptrs") and its sums to the values ("value bits").  `for w0`, the write-out: with n = 8300 the second round
  writes behind `run`; without the running offset it overwrites the row's head: "cols" fails.
* spgemm_products_kernel, `for base` (C): stopped after one trip, work[] of rows 16 384 .. is unset, so those rows are
  classed by what the allocation held ("row_ptrs" fails where that is no product count), and the totals lack them:
  res.products (the host test: the first trip's sum differs) and res.max_row_products (the 800 of row 16 386) fail.
* spgemm_classify_kernel (D) has no loop; its flag index is blockIdx.x % kMaxGrid.  A class-0 row is in no list but
  list 0, and launch_pass (spgemm.hip:611) starts at class 1, so no other kernel visits row m - 1: without the classify
  flag the call returns 0 and error_code == INVALID_FORMAT fails.
* matrix_bad of spgemm_validate_kernel (E) and the loop of transpose_validate_kernel (F): stopped after one trip, or
  striding too far, work item nnz - 1 (or m - 1) is never taken, the call is not rejected: error_code == INVALID_FORMAT
  fails.  F's `diff`: without the second trip's contribution no pass runs and the result is A's arrays in A's order:
  "row_ptrs" of the comparison with numpy's stable transpose fails (the host test: they differ).

No case makes a kernel follow a bad index: begin() (spgemm.hip:670) returns on validate()'s status before the products
kernel is launched, transpose_build (transpose.hip:231) before anything is allocated; the validation kernels read
row_ptrs[0 .. rows] and cols[0 .. nnz) only, and the search of the order check stays inside row_ptrs.  D's two patterns
are well formed (the host test); their kernels index C and A through row pointers that stay inside both."""
import ctypes

import numpy as np
import pytest

import spgemm_cases as sc
import spgemm_trip_cases as tc
from test_gpu_transpose import np_transpose

pytestmark = pytest.mark.gpu

FIELDS = ("products", "max_row_products", "nnz", "max_row_nnz")


# ---- helpers ----------------------------------------------------------------------------------------------------------
def _upload(gpu, rows, cols, arrays):
    M = gpu.csr_from_arrays(rows, cols, *arrays)
    assert gpu.csr_to_gpu(M) == 0
    return M


def _download(gpu, C):
    assert gpu.csr_from_gpu(C) == 0
    return gpu.csr_host_arrays(C)


def _words(gpu, address, count):
    out = np.empty(count, np.uint32)
    if count:
        assert gpu.lib().spmv_c_memcpy_d2h(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(address), 4 * count) == 0
    return out


def _put(gpu, address, array):
    array = np.ascontiguousarray(array)
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(address), array.ctypes.data_as(ctypes.c_void_p), array.nbytes) == 0


def _int_buffer(gpu, values):
    values = np.ascontiguousarray(values, np.int32)
    buf = gpu.CudaBuffer(values.size, "int32")
    buf.copyFromHost(values, values.size)
    return buf


def _twin(gpu, A, B):
    H = gpu.csr_create(0, 0, 0)
    assert gpu.spgemm_cpu_csr(H, A, B) == 0
    got = gpu.csr_host_arrays(H)
    gpu.csr_destroy(H)
    return got


def _seven(C):
    m = C.contents
    return (m.num_rows, m.num_cols, m.nnz, bool(m.owns_device_memory), m.d_row_ptrs, m.d_col_indices, m.d_values)


class Pair:
    """A and B on the device with the judge's C, the second witness's C, and the same for A's other values"""

    def __init__(self, gpu, case, want, want2=None):
        self.gpu, self.case, self.want, self.want2 = gpu, case, want, want2
        self.m, self.k, self.n = case["m"], case["k"], case["n"]
        self.A, self.B = _upload(gpu, self.m, self.k, case["a"]), _upload(gpu, self.k, self.n, case["b"])
        self.twin = _twin(gpu, self.A, self.B)
        sc.assert_same(self.twin, want, "spgemm_cpu_csr against the reference")
        self.twin2 = None
        if want2 is not None:
            A2 = gpu.csr_from_arrays(self.m, self.k, *case["a2"])
            self.twin2 = _twin(gpu, A2, self.B)
            gpu.csr_destroy(A2)
            sc.assert_same(self.twin2, want2, "spgemm_cpu_csr against the reference, other values")
        for mat in (want, want2, self.twin, self.twin2, case["a"], case["b"]):
            for array in mat or ():
                array.setflags(write=False)

    def fields(self, forced=0):
        return tc.expected_fields(self.case["a"], self.case["b"], self.want[0], self.n, forced)

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.gpu.csr_destroy(self.B)


def _build(gpu, P, forced, what, lanes=None):
    """spgemm_csr(A, B): C's handle, after every comparison"""
    C = gpu.csr_create(3, 3, 2)
    res = gpu.spgemm_csr(C, P.A, P.B)
    assert res.error_code == 0, (what, res.error_code)
    assert (C.contents.num_rows, C.contents.num_cols) == (P.m, P.n) and C.contents.owns_device_memory
    got = _download(gpu, C)
    sc.assert_same(got, P.want, f"{what}: against the reference")
    sc.assert_same(got, P.twin, f"{what}: against spgemm_cpu_csr")
    want = P.fields(forced)
    assert {f: getattr(res, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    assert list(res.symbolic_rows) == want["symbolic_rows"], (what, list(res.symbolic_rows))
    assert list(res.numeric_rows) == want["numeric_rows"], (what, list(res.numeric_rows))
    assert lanes is None or res.lanes == lanes
    return C


def _refill(gpu, P, C, forced, what, lanes=None):
    """spgemm_csr_numeric into C after A's device values were overwritten and C's replaced by a sentinel"""
    m = C.contents
    structure = (_words(gpu, m.d_row_ptrs, m.num_rows + 1), _words(gpu, m.d_col_indices, m.nnz))
    _put(gpu, P.A.contents.d_values, P.case["a2"][2])
    _put(gpu, m.d_values, np.full(m.nnz, tc.SENTINEL, np.uint32))
    try:
        res = gpu.spgemm_csr_numeric(C, P.A, P.B)
        assert res.error_code == 0, (what, res.error_code)
        got = _download(gpu, C)
        sc.assert_same(got, P.want2, f"{what}: values only, against the reference")
        sc.assert_same(got, P.twin2, f"{what}: values only, against spgemm_cpu_csr")
        after = (_words(gpu, m.d_row_ptrs, m.num_rows + 1), _words(gpu, m.d_col_indices, m.nnz))
        assert structure[0].tobytes() == after[0].tobytes() and structure[1].tobytes() == after[1].tobytes(), what
        want = P.fields(forced)
        assert (res.products, res.max_row_products, res.nnz) == (want["products"], want["max_row_products"], want["nnz"])
        assert list(res.numeric_rows) == want["numeric_rows"] and sum(res.symbolic_rows) == 0, what
        assert lanes is None or res.lanes == lanes
    finally:
        _put(gpu, P.A.contents.d_values, P.case["a"][2])


# ---- A: every geometry --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry(gpu):
    case = tc.geometry_case()
    P = Pair(gpu, case, sc.product_loop(case["m"], case["n"], case["a"], case["b"]),
             sc.product_loop(case["m"], case["n"], case["a2"], case["b"]))
    yield P
    P.close()


GEOMETRIES = [(cls, lanes) for cls in (1, 2, 3) for lanes in tc.LANES] + [(4, 1), (4, 64), (5, 1), (5, 64)]


@pytest.mark.parametrize("cls,lanes", GEOMETRIES)
def test_a_every_class_at_every_lane_count_in_every_pass(gpu, monkeypatch, geometry, cls, lanes):
    P = geometry
    what = f"class {cls}, {lanes} lanes"
    monkeypatch.setenv("SPMV_DEBUG", f"spgemm_class={cls},spgemm_lanes={lanes}")
    C = None
    try:
        C = _build(gpu, P, cls, what, lanes)
        want = P.fields(cls)
        distinct = tc.row_lengths(P.want[0])
        fits = (distinct > 0) & (distinct <= (tc.CAPS[cls - 1] if cls < 5 else 2**31))
        assert want["numeric_rows"][cls] == fits.sum() and want["numeric_rows"][0] == (distinct == 0).sum()
        _refill(gpu, P, C, cls, what, lanes)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(C)


# ---- B: second trips of the table and dense kernels ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def trip_pairs(gpu):
    made = {}

    def get(n):
        if n not in made:
            case = tc.trip_case(n)
            made[n] = Pair(gpu, case, tc.trip_reference(case), tc.trip_reference(case, "period2"))
        return made[n]
    yield get
    for P in made.values():
        P.close()


@pytest.mark.parametrize("forced,n", [(0, tc.TRIP_N[0]), (2, tc.TRIP_N[0]), (3, tc.TRIP_N[0]), (4, tc.TRIP_N[0]),
                                      (5, tc.TRIP_N[0]), (5, tc.TRIP_N[1])])
def test_b_later_trips_of_the_table_and_dense_kernels(gpu, monkeypatch, trip_pairs, forced, n):
    P = trip_pairs(n)
    what = f"forced class {forced}, n = {n}"
    monkeypatch.setenv("SPMV_DEBUG", f"spgemm_lanes=64,spgemm_class={forced}")
    C = None
    try:
        C = _build(gpu, P, forced, what, 64)
        assert P.fields(forced)["numeric_rows"][max(forced, 1)] == P.m == tc.TRIP_ROWS
        _refill(gpu, P, C, forced, what, 64)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(C)


# ---- C: the products kernel at 64 lanes per row of A ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def products(gpu):
    case = tc.products_case()
    want, bound = tc.integer_product(case["m"], case["k"], case["n"], case["a"], case["b"])
    assert bound < 2**24
    P = Pair(gpu, case, want)
    yield P
    P.close()


def test_c_the_products_kernel_makes_a_second_trip_at_64_lanes(gpu, products):
    P = products
    a = P.case["a"]
    assert tc.pick_lanes(a[1].size, P.m) == 64 and P.m > 4 * tc.MAX_GRID
    C = _build(gpu, P, 0, "products", tc.pick_lanes(P.case["b"][1].size, P.k))
    work = tc.row_products(a, P.case["b"])
    want = P.fields()
    assert want["products"] == int(work.sum()) and want["max_row_products"] == int(work[tc.PRODUCTS_LONG_ROW]) == 800
    gpu.csr_destroy(C)


# ---- D: the classify flag alone, from workgroup 4097 ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def classify(gpu):
    case = tc.classify_case()
    P = Pair(gpu, case, tc.classify_reference(case))
    yield P
    P.close()


def test_d_a_row_with_products_and_no_entries_or_the_reverse_is_rejected_by_the_classify_flag_alone(gpu, classify):
    """Row m - 1 is classified by workgroup 4097 of spgemm_classify_kernel, which raises flags[4097 % 4096].  The row
    lands in class 0 (its key or its products are 0); launch_pass runs classes 1 .. 5 only and the lists of those
    classes hold no class-0 row, so no table or dense kernel visits it: the classify flag is the only source of the
    rejection.  Every other row is intact and its refill legitimate, so C's values are rewritten with the same bits."""
    E = gpu.SpMVError
    P = classify
    m, n, k = P.m, P.n, P.k
    C = _build(gpu, P, 0, "classify")
    a_nnz, c_nnz = P.A.contents.nnz, C.contents.nnz
    assert gpu.spgemm_csr_numeric(C, P.A, P.B).error_code == 0
    good = _words(gpu, C.contents.d_values, c_nnz)
    assert good.tobytes() == sc.bits(P.want[2]).tobytes()
    bufs = []
    try:
        # products and no entries: C without its last entry, through a copy of its row pointers
        rp = P.want[0].copy()
        rp[m] = c_nnz - 1
        bufs.append(_int_buffer(gpu, rp))
        cut = gpu.csr_wrap_device(m, n, c_nnz - 1, bufs[-1].get(), C.contents.d_col_indices, C.contents.d_values)
        res = gpu.spgemm_csr_numeric(cut, P.A, P.B)
        gpu.csr_destroy(cut)
        assert res.error_code == E.INVALID_FORMAT
        assert _words(gpu, C.contents.d_values, c_nnz).tobytes() == good.tobytes()
        # entries and no products: A without its last entry
        rp = P.case["a"][0].copy()
        rp[m] = a_nnz - 1
        bufs.append(_int_buffer(gpu, rp))
        cut = gpu.csr_wrap_device(m, k, a_nnz - 1, bufs[-1].get(), P.A.contents.d_col_indices, P.A.contents.d_values)
        res = gpu.spgemm_csr_numeric(C, cut, P.B)
        gpu.csr_destroy(cut)
        assert res.error_code == E.INVALID_FORMAT
        assert _words(gpu, C.contents.d_values, c_nnz).tobytes() == good.tobytes()
        # and the intact matrices pass again
        assert gpu.spgemm_csr_numeric(C, P.A, P.B).error_code == 0
        assert _words(gpu, C.contents.d_values, c_nnz).tobytes() == good.tobytes()
    finally:
        for buf in bufs:
            buf.release()
        gpu.csr_destroy(C)


# ---- E: spgemm_validate_kernel past its first trip ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scaled(gpu):
    case = tc.scaled_rows_case()
    P = Pair(gpu, case, tc.scaled_rows_reference(case))
    yield P
    P.close()


def _rejected_untouched(gpu, A, B, name):
    C = gpu.csr_create(2, 3, 1)
    before = _seven(C)
    status = gpu.spgemm_csr(C, A, B).error_code
    after = _seven(C)
    gpu.csr_destroy(C)
    assert status == gpu.SpMVError.INVALID_FORMAT, (name, status)
    assert after == before, name


def test_e_defects_of_a_past_the_first_trip(gpu, products, classify):
    P = products
    a, nnz = P.case["a"], P.A.contents.nnz
    assert nnz - 1 >= tc.VALIDATE_ITEMS
    gpu.csr_destroy(_build(gpu, P, 0, "A without a defect"))
    for name, bad in tc.column_defects(a[1], P.k, False).items():
        buf = _int_buffer(gpu, bad)
        A = gpu.csr_wrap_device(P.m, P.k, nnz, P.A.contents.d_row_ptrs, buf.get(), P.A.contents.d_values)
        try:
            _rejected_untouched(gpu, A, P.B, name)
        finally:
            gpu.csr_destroy(A)
            buf.release()
    # a decreasing pair of row pointers at the last row of D's matrix: work item m - 1 of 1 048 877
    D = classify
    rp = D.case["a"][0].copy()
    rp[D.m - 1] = D.A.contents.nnz + 1
    buf = _int_buffer(gpu, rp)
    A = gpu.csr_wrap_device(D.m, D.k, D.A.contents.nnz, buf.get(), D.A.contents.d_col_indices, D.A.contents.d_values)
    try:
        _rejected_untouched(gpu, A, D.B, "A's row pointers decrease at the last row")
    finally:
        gpu.csr_destroy(A)
        buf.release()
    gpu.csr_destroy(_build(gpu, D, 0, "D's matrix without a defect"))


def test_e_defects_of_b_and_of_c_past_the_first_trip(gpu, scaled):
    E = gpu.SpMVError
    P = scaled
    b, nnz = P.case["b"], P.B.contents.nnz
    assert nnz - 1 >= tc.VALIDATE_ITEMS
    C = _build(gpu, P, 0, "B without a defect", tc.pick_lanes(nnz, P.k))
    try:
        for name, bad in tc.column_defects(b[1], P.n, True).items():
            buf = _int_buffer(gpu, bad)
            B = gpu.csr_wrap_device(P.k, P.n, nnz, P.B.contents.d_row_ptrs, buf.get(), P.B.contents.d_values)
            try:
                _rejected_untouched(gpu, P.A, B, name)
            finally:
                gpu.csr_destroy(B)
                buf.release()
        # C in the values-only pass: its last column out of range, through a copy of its columns
        c_nnz = C.contents.nnz
        assert c_nnz - 1 >= tc.VALIDATE_ITEMS
        assert gpu.spgemm_csr_numeric(C, P.A, P.B).error_code == 0
        good = _words(gpu, C.contents.d_values, c_nnz)
        assert good.tobytes() == sc.bits(P.want[2]).tobytes()
        for name, bad in tc.column_defects(P.want[1], P.n, False).items():
            buf = _int_buffer(gpu, bad)
            W = gpu.csr_wrap_device(P.m, P.n, c_nnz, C.contents.d_row_ptrs, buf.get(), C.contents.d_values)
            try:
                assert gpu.spgemm_csr_numeric(W, P.A, P.B).error_code == E.INVALID_FORMAT, name
                assert _words(gpu, C.contents.d_values, c_nnz).tobytes() == good.tobytes(), name
            finally:
                gpu.csr_destroy(W)
                buf.release()
    finally:
        gpu.csr_destroy(C)


# ---- F: transpose_validate_kernel past its first trip ---------------------------------------------------------------------
def _same_bytes(got, want, what):
    for g, w, part in zip(got, want, ("row_ptrs", "col_indices", "values")):
        assert np.asarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, part)


@pytest.mark.parametrize("variant", list(tc.TRANSPOSE_VARIANTS))
def test_f_a_second_trip_entry_alone_decides_a_radix_pass(gpu, variant):
    rows, cols, (rp, ci, va) = tc.transpose_case(tc.TRANSPOSE_VARIANTS[variant])
    A, T = _upload(gpu, rows, cols, (rp, ci, va)), gpu.csr_create(3, 3, 2)
    try:
        assert gpu.csr_transpose_gpu(T, A) == 0
        assert (T.contents.num_rows, T.contents.num_cols, T.contents.nnz) == (cols, rows, ci.size)
        want = np_transpose(rows, cols, rp, ci, va)
        _same_bytes(_download(gpu, T), want, variant)
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(T)


def test_f_defects_at_the_last_entry_are_rejected_with_no_output(gpu):
    E = gpu.SpMVError
    rows, cols, (rp, ci, va) = tc.transpose_case((8, 16))
    T = gpu.csr_create(2, 3, 1)
    before = _seven(T)
    for name, bad in tc.column_defects(ci, cols, False).items():
        A = _upload(gpu, rows, cols, (rp, bad, va))
        status = gpu.csr_transpose_gpu(T, A)
        gpu.csr_destroy(A)
        assert status == E.INVALID_FORMAT, (name, status)
        assert _seven(T) == before, name
    gpu.csr_destroy(T)
