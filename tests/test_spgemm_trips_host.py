"""What every case of tests/test_gpu_spgemm_trips.py is named for, proved without a GPU (tests/spgemm_trip_cases.py):
the cap each case passes, from the launch arithmetic of csrc/spgemm.hip and csrc/transpose.hip restated; that the rows
of a later trip are no copies of the rows one stride above them; that every row meets the class conditions the case
claims; and that the tiled or integer reference equals spgemm_cpu_csr on the whole matrix and
spgemm_cases.product_loop, the definition, on the period."""
import numpy as np
import pytest

import spgemm_cases as sc
import spgemm_trip_cases as tc
from test_gpu_transpose import np_transpose


def _host(spmv, case, a=None):
    status, got = sc.host_product(spmv, case["m"], case["k"], case["n"], case["a"] if a is None else a, case["b"])
    assert status == 0
    return got


def _row_set(mat):
    """every row as (columns, value bits)"""
    rp, ci, va = mat
    return [(ci[rp[i]:rp[i + 1]].tobytes(), sc.bits(va[rp[i]:rp[i + 1]]).tobytes()) for i in range(rp.size - 1)]


def _visits(count, per_workgroup, grid, stride, first_trip_only=False):
    """how often each of `count` list positions is taken by a grid-stride loop `for base = block * per; base < count;
    base += stride` whose workgroups take `per_workgroup` positions from base on"""
    seen = np.zeros(count, np.int64)
    for block in range(grid):
        base = block * per_workgroup
        while base < count:
            seen[base:min(base + per_workgroup, count)] += 1
            if first_trip_only:
                break
            base += stride
    return seen


# ---- the restated launch arithmetic -----------------------------------------------------------------------------------
def test_the_geometries_of_the_table_kernel():
    """threads per workgroup = tables * lanes, as launch_tables sizes them"""
    for lanes in tc.LANES:
        for symbolic in (True, False):
            assert tc.tables(1, lanes, symbolic) == 256 // lanes and tc.workgroup_threads(1, lanes, symbolic) == 256
            assert tc.tables(4, lanes, symbolic) == 1 and tc.workgroup_threads(4, lanes, symbolic) == 256
        assert tc.tables(2, lanes, True) == min(256 // lanes, 64) and tc.tables(2, lanes, False) == min(256 // lanes, 32)
        assert tc.tables(3, lanes, True) == min(256 // lanes, 8) and tc.tables(3, lanes, False) == min(256 // lanes, 4)
    assert [tc.workgroup_threads(2, L, True) for L in (1, 2, 4, 8)] == [64, 128, 256, 256]
    assert [tc.workgroup_threads(2, L, False) for L in (1, 2, 4, 8, 16)] == [32, 64, 128, 256, 256]
    assert [tc.workgroup_threads(3, L, True) for L in tc.LANES] == [8, 16, 32, 64, 128, 256, 256]
    assert [tc.workgroup_threads(3, L, False) for L in tc.LANES] == [4, 8, 16, 32, 64, 128, 256]
    # lanes: 1 up to a mean of 4, 2 up to 8, ... 64 above 128
    assert [tc.pick_lanes(x, 1) for x in (0, 4, 5, 8, 9, 128, 129, 10_000)] == [1, 1, 2, 2, 4, 32, 64, 64]
    assert [tc.class_of(x) for x in (0, 1, 16, 17, 128, 129, 1024, 1025, 8192, 8193)] == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert tc.class_of(3, 4) == 4 and tc.class_of(200, 2) == 3 and tc.class_of(0, 5) == 0
    keys = np.arange(0, 9000, 7)
    for forced in range(6):
        want = np.bincount([tc.class_of(int(x), forced) for x in keys], minlength=8).tolist()
        assert tc.histogram(keys, forced) == want


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    return tc.geometry_case()


def test_a_the_geometry_matrix_is_what_it_claims(spmv, geometry):
    g = geometry
    m, n, a, b = g["m"], g["n"], g["a"], g["b"]
    want = sc.product_loop(m, n, a, b)
    sc.assert_same(_host(spmv, g), want, "A")
    sc.assert_same(_host(spmv, g, g["a2"]), sc.product_loop(m, n, g["a2"], b), "A, other values")
    assert np.all(sc.bits(g["a2"][2]) != sc.bits(a[2]))
    distinct, products = tc.row_lengths(want[0]), tc.row_products(a, b)
    assert 300 <= m <= 340 and n % 32 != 0
    assert sorted(set(tc.row_lengths(b[0]).tolist())) == tc.GEOMETRY_LENGTHS          # L - 1, L, L + 1, 2 L + 1
    assert set(range(0, 17)) <= set(distinct.tolist()) and ((distinct > 16) & (distinct <= 40)).sum() >= 10
    assert distinct.max() >= 129 and products.max() <= 1024                           # nothing past class 3 by itself
    # two overlapping B rows: the symbolic key is larger than the numeric one, for some rows by a whole class
    assert (np.minimum(products, n) > distinct).sum() >= 19
    sym = [tc.class_of(int(min(p, n))) for p in products]
    num = [tc.class_of(int(d)) for d in distinct]
    assert sum(s > c for s, c in zip(sym, num)) >= 2
    # A unsorted, with repeats; some rows have entries and no products
    lengths = tc.row_lengths(a[0])
    starts = a[0][:-1][lengths >= 2]
    assert (a[1][starts + 1] < a[1][starts]).any()
    assert any(np.unique(a[1][a[0][i]:a[0][i + 1]]).size < lengths[i] for i in range(m))
    assert ((lengths > 0) & (products == 0)).any() and (lengths == 0).any()
    # forced class 1: more rows than the 256 tables of one workgroup at one lane, the last workgroup partial
    f1 = tc.expected_fields(a, b, want[0], n, 1)
    for hist in (f1["symbolic_rows"], f1["numeric_rows"]):
        assert hist[1] > 256 and hist[1] % 256 != 0 and hist[2] > 0 and hist[0] > 0
        assert tc.table_grid(hist[1], 1, 1, False) == 2
    # forced classes 2 .. 5: every non-empty row that fits is in the forced class
    for forced in (2, 3, 4, 5):
        f = tc.expected_fields(a, b, want[0], n, forced)
        cap = tc.CAPS[forced - 1] if forced < 5 else 2**31
        assert f["numeric_rows"][forced] == ((distinct > 0) & (distinct <= cap)).sum() > 256
        assert f["symbolic_rows"][forced] == ((products > 0) & (np.minimum(products, n) <= cap)).sum() > 256
        assert f["numeric_rows"][0] == (distinct == 0).sum() and sum(f["numeric_rows"]) == m
        if forced >= 3:
            assert f["numeric_rows"][forced] == (distinct > 0).sum() == f["symbolic_rows"][forced]
        # every class below class 4 runs more than one workgroup at every lane count, in both passes
        if forced < 4:
            for lanes in tc.LANES:
                assert tc.table_grid(f["numeric_rows"][forced], forced, lanes, False) >= 2
                assert tc.table_grid(f["symbolic_rows"][forced], forced, lanes, True) >= 2


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.TRIP_N)
def test_b_the_trip_matrix_passes_every_cap_it_is_named_for(spmv, n):
    case = tc.trip_case(n)
    m, a, b = case["m"], case["a"], case["b"]
    assert m == 4 * tc.MAX_GRID + 7
    # classes 1 .. 3 at 64 lanes: four tables a workgroup in both passes, 4096 workgroups, a second trip of 7 rows
    for cls in (1, 2, 3):
        for symbolic in (True, False):
            assert tc.tables(cls, 64, symbolic) == 4
            assert tc.table_grid(m, cls, 64, symbolic) == tc.MAX_GRID < tc.trips(m, 4)
    seen = _visits(m, 4, tc.MAX_GRID, 4 * tc.MAX_GRID)
    assert np.all(seen == 1)
    once = _visits(m, 4, tc.MAX_GRID, 4 * tc.MAX_GRID, first_trip_only=True)
    assert np.flatnonzero(once == 0).tolist() == list(range(4 * tc.MAX_GRID, m))      # 4 rows of workgroup 0, 3 of 1
    assert np.any(_visits(m, 4, tc.MAX_GRID, 8 * tc.MAX_GRID) == 0)                   # a stride too long skips rows
    # class 4: one table a workgroup, five trips; the dense class: 256 slices, 65 trips
    assert tc.tables(4, 64, False) == 1 and tc.trips(m, tc.MAX_GRID) == 5
    assert tc.trips(m, tc.DENSE_GROUPS) == 65
    words = (n + 31) // 32
    assert n % 32 != 0 and (words < tc.THREADS if n < 8192 else tc.THREADS < words <= 2 * tc.THREADS)
    # every row is class 1 by itself in both passes
    period_c = sc.product_loop(tc.TRIP_PERIOD, n, case["period"], b)
    want = tc.tile_rows(period_c, m)
    products, distinct = tc.row_products(a, b), tc.row_lengths(want[0])
    assert products.min() >= 1 and products.max() <= 16 and distinct.min() >= 1
    f = tc.expected_fields(a, b, want[0], n)
    assert f["symbolic_rows"] == f["numeric_rows"] == [0, m, 0, 0, 0, 0, 0, 0]
    for forced in (2, 3, 4, 5):
        f = tc.expected_fields(a, b, want[0], n, forced)
        assert f["symbolic_rows"][forced] == f["numeric_rows"][forced] == m
    # no two period rows are equal and no stride is a multiple of the period: a row of a later trip differs from the
    # row one stride above it, in A and in C, with both sets of values
    for stride in (4 * tc.MAX_GRID, tc.MAX_GRID, tc.DENSE_GROUPS):
        assert stride % tc.TRIP_PERIOD != 0
    for which in ("period", "period2"):
        c = sc.product_loop(tc.TRIP_PERIOD, n, case[which], b)
        assert len(set(_row_set(c))) == tc.TRIP_PERIOD and len(set(_row_set(case[which]))) == tc.TRIP_PERIOD
    rows_a, rows_c = _row_set(a), _row_set(want)
    for stride in (4 * tc.MAX_GRID, tc.MAX_GRID, tc.DENSE_GROUPS):
        assert all(rows_a[i] != rows_a[i - stride] and rows_c[i] != rows_c[i - stride] for i in range(stride, m))
    # the references: the tiled one on the whole matrix, the definition on the period
    sc.assert_same(_host(spmv, case), want, "B")
    sc.assert_same(_host(spmv, case, case["a2"]), tc.trip_reference(case, "period2"), "B, other values")
    status, got = sc.host_product(spmv, tc.TRIP_PERIOD, case["k"], n, case["period"], b)
    assert status == 0
    sc.assert_same(got, period_c, "B, the period")
    # the dense write-out: with n > 8192 some row has columns on both sides of map word 256, so the second round of the
    # write-out loop starts at a running offset that is not 0
    low = np.minimum.reduceat(want[1], want[0][:-1]) < 8192
    high = np.maximum.reduceat(want[1], want[0][:-1]) >= 8192
    assert bool((low & high).any()) == (n > 8192) and want[1].max() == n - 1 and want[1].min() == 0


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def products():
    return tc.products_case()


def test_c_the_products_matrix_passes_the_cap_and_is_exact(spmv, products):
    case = products
    m, k, n, a, b = case["m"], case["k"], case["n"], case["a"], case["b"]
    nnz = a[1].size
    assert m == 4 * tc.MAX_GRID + 5 and nnz / m > 128 and nnz > 2_000_000
    a_lanes = tc.pick_lanes(nnz, m)
    per = tc.THREADS // a_lanes
    assert a_lanes == 64 and per == 4 and tc.trips(m, per) > tc.MAX_GRID
    assert np.all(_visits(m, per, tc.MAX_GRID, per * tc.MAX_GRID) == 1)
    assert (_visits(m, per, tc.MAX_GRID, tc.MAX_GRID) > 1).any()          # striding by the grid alone counts rows twice
    work = tc.row_products(a, b)
    assert work.argmax() == tc.PRODUCTS_LONG_ROW >= per * tc.MAX_GRID and work.max() == 800
    assert np.sort(work)[-2] < 800                                       # the maximum sits in the second trip alone
    second = np.arange(per * tc.MAX_GRID, m)
    assert np.all(work[second] != work[second - per * tc.MAX_GRID])
    assert work[:per * tc.MAX_GRID].sum() != work.sum()
    assert set(tc.row_lengths(b[0]).tolist()) == {1, 2} and tc.pick_lanes(b[1].size, k) == 1
    # exact in fp32 in any order, every output column a sum of a dozen terms or more
    want, bound = tc.integer_product(m, k, n, a, b)
    assert bound < 2**24
    terms = np.zeros((m, n), np.int64)
    b_rows = tc.rows_of(b[0])
    for r, c in zip(b_rows.tolist(), b[1].tolist()):
        terms[:, c] += np.bincount(tc.rows_of(a[0])[a[1] == r], minlength=m)
    assert terms[terms > 0].min() >= 12
    sc.assert_same(_host(spmv, case), want, "C")
    some = np.asarray([0, 1, tc.PRODUCTS_LONG_ROW, m - 1])
    pick = np.concatenate([np.arange(a[0][i], a[0][i + 1]) for i in some])
    few = (np.concatenate([[0], np.cumsum(tc.row_lengths(a[0])[some])]).astype(np.int32), a[1][pick], a[2][pick])
    loop = sc.product_loop(some.size, n, few, b)
    for j, i in enumerate(some):
        assert _row_set(loop)[j] == _row_set(want)[i]
    f = tc.expected_fields(a, b, want[0], n)
    assert f["symbolic_rows"] == f["numeric_rows"] == [0, m, 0, 0, 0, 0, 0, 0]
    assert f["products"] == int(work.sum()) and f["max_row_products"] == 800 and f["max_row_nnz"] <= n


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def classify():
    return tc.classify_case()


def test_d_the_classify_matrix_raises_the_flag_from_workgroup_4097_alone(spmv, classify):
    case = classify
    m, n, a, b, at = case["m"], case["n"], case["a"], case["b"], case["at"]
    assert m == tc.MAX_GRID * tc.THREADS + 300 and tc.trips(m, tc.THREADS) == tc.MAX_GRID + 2
    assert (m - 1) // tc.THREADS == tc.MAX_GRID + 1 and ((m - 1) // tc.THREADS) % tc.MAX_GRID == 1
    assert 30 <= at.size <= 40 and at[0] == 0 and at[-1] == m - 1 and (at >= tc.MAX_GRID * tc.THREADS).sum() >= 5
    want = tc.classify_reference(case)
    sc.assert_same(_host(spmv, case), want, "D")
    c_rp, c_nnz, a_nnz = want[0], want[1].size, a[1].size
    work, distinct = tc.row_products(a, b), tc.row_lengths(c_rp)
    assert np.array_equal(work > 0, distinct > 0)
    assert tc.row_lengths(a[0])[m - 9] == 1 and work[m - 9] == 0          # entries of A and no products: class 0
    assert distinct[m - 1] == 1 and tc.row_lengths(a[0])[m - 1] == 1 and work[m - 1] == 1
    # C with its last entry cut off: well formed, and the last row alone has products and no entries
    cut = c_rp.copy()
    cut[m] = c_nnz - 1
    assert tc.items_that_see(cut, want[1], c_nnz - 1, n, False) == []
    assert np.flatnonzero((tc.row_lengths(cut) > 0) != (work > 0)).tolist() == [m - 1]
    # A with its last entry cut off: well formed, and C's last row alone has entries and no products
    cut = a[0].copy()
    cut[m] = a_nnz - 1
    assert tc.items_that_see(cut, a[1], a_nnz - 1, case["k"], False) == []
    cut_work = tc.row_products((cut, a[1][:-1], a[2][:-1]), b)
    assert np.flatnonzero((distinct > 0) != (cut_work > 0)).tolist() == [m - 1]
    # E's decreasing pair of row pointers: seen by work item m - 1 alone, in the third trip of the check
    down = a[0].copy()
    down[m - 1] = a_nnz + 1
    assert tc.items_that_see(down, a[1], a_nnz, case["k"], False) == [m - 1] and m - 1 >= 2 * tc.VALIDATE_ITEMS
    assert tc.expected_fields(a, b, c_rp, n)["numeric_rows"][:2] == [m - (distinct > 0).sum(), (distinct > 0).sum()]


# ---- E ------------------------------------------------------------------------------------------------------------------
def test_e_every_defect_is_seen_by_one_work_item_past_the_first_trip(spmv, products):
    case = tc.scaled_rows_case()
    m, n, a, b = case["m"], case["n"], case["a"], case["b"]
    b_nnz = b[1].size
    assert b_nnz == tc.VALIDATE_ITEMS + 600 and tc.trips(b_nnz, tc.THREADS) > tc.VALIDATE_GRID
    assert tc.items_that_see(b[0], b[1], b_nnz, n, True) == [] and tc.items_that_see(a[0], a[1], m, m, False) == []
    defects = tc.column_defects(b[1], n, True)
    assert len(defects) == 3
    for name, bad in defects.items():
        assert tc.items_that_see(b[0], bad, b_nnz, n, True) == [b_nnz - 1], name
    assert b[1][-1] != b[1][-2] and defects["a descending pair at the end of the last row"][-1] >= 0
    want = tc.scaled_rows_reference(case)
    sc.assert_same(_host(spmv, case), want, "E")
    few = (a[0][:41], a[1][:40], a[2][:40])
    loop = sc.product_loop(40, n, few, b)
    sc.assert_same(loop, (want[0][:41], want[1][:320], want[2][:320]), "E, the first rows by the definition")
    f = tc.expected_fields(a, b, want[0], n)
    assert f["symbolic_rows"] == f["numeric_rows"] == [0, m, 0, 0, 0, 0, 0, 0] and f["nnz"] == b_nnz
    # C's own defect in the values-only pass
    for name, bad in tc.column_defects(want[1], n, False).items():
        assert tc.items_that_see(want[0], bad, b_nnz, n, False) == [b_nnz - 1], name
    # A's defects, on the matrix of C: more than two million entries
    pa, k = products["a"], products["k"]
    a_nnz = pa[1].size
    assert tc.items_that_see(pa[0], pa[1], a_nnz, k, False) == [] and a_nnz - 1 >= 4 * tc.VALIDATE_ITEMS
    for name, bad in tc.column_defects(pa[1], k, False).items():
        assert tc.items_that_see(pa[0], bad, a_nnz, k, False) == [a_nnz - 1], name


# ---- F ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(tc.TRANSPOSE_VARIANTS))
def test_f_one_second_trip_entry_decides_each_radix_pass(variant):
    bits = tc.TRANSPOSE_VARIANTS[variant]
    rows, cols, (rp, ci, va) = tc.transpose_case(bits)
    nnz = ci.size
    assert nnz == tc.VALIDATE_ITEMS + 600 and rp[-1] == nnz and cols > 65536 + tc.TRANSPOSE_C0
    assert np.all(ci[:tc.VALIDATE_ITEMS] == tc.TRANSPOSE_C0)              # the first trip sees one column only
    assert tc.radix_digits(ci[:tc.VALIDATE_ITEMS]) == []
    assert tc.radix_digits(ci) == [bit // 8 for bit in bits]
    other = np.flatnonzero(ci != tc.TRANSPOSE_C0)
    assert other.tolist() == [tc.TRANSPOSE_AT[bit] for bit in bits] and other.min() >= tc.VALIDATE_ITEMS
    for bit in bits:
        assert int(ci[tc.TRANSPOSE_AT[bit]]) ^ tc.TRANSPOSE_C0 == 1 << bit
    assert other.max() < nnz - 1                                          # entries of column 5 follow: the sort moves them
    # a transpose that skipped the passes differs from the stable one in row pointers and in columns
    t_rp, t_ci, t_va = np_transpose(rows, cols, rp, ci, va)
    assert np.diff(t_rp).max() == nnz - len(bits) and (np.diff(t_rp) == 1).sum() == len(bits)
    assert not np.array_equal(t_ci, tc.rows_of(rp).astype(np.int32))
    assert tc.items_that_see(rp, ci, nnz, cols, False) == []
    for name, bad in tc.column_defects(ci, cols, False).items():
        assert tc.items_that_see(rp, bad, nnz, cols, False) == [nnz - 1], name
