"""Generators and CPU provers for the trip and geometry tests of spgemm_csr (csrc/spgemm.hip) and of
the transpose's structure check (csrc/transpose.hip): tests/test_spgemm_trips_host.py proves what each case is named
for, tests/test_gpu_spgemm_trips.py runs them.

numpy only; the library is never imported here.  A matrix is (row_ptrs int32, cols int32, vals float32).

* the launch arithmetic of spgemm.hip restated: pick_lanes, class_of, tables, workgroup_threads, table_grid, trips.
* expected_fields: products, max_row_products, nnz, max_row_nnz and both class histograms from numpy.
* tile_rows: a period of rows repeated down a matrix; the large expected products are tiled periods of
  spgemm_cases.product_loop, the definition.
* geometry_case (A), trip_case (B), products_case (C), classify_case (D), scaled_rows_case (E), transpose_case (F).
* items_that_see: the work items of matrix_bad (spgemm_validate_kernel) that find something wrong.
A plain module, not a conftest."""
import numpy as np

import spgemm_cases as sc

THREADS = 256                        # kThreads, spgemm.hip:31 and transpose.hip:28
MAX_GRID = 4096                      # kMaxGrid, spgemm.hip:32
TABLE_BUDGET = 64 * 1024             # kTableBudget, spgemm.hip:35
SLOTS = (32, 256, 2048, 16384)       # kSpgemmSlots / slots_of, spgemm.hip:37-39; a table is at most half full
CAPS = tuple(s // 2 for s in SLOTS)
CLASSES = 5                          # kSpgemmClasses: four tables and the dense class
DENSE_GROUPS = 256                   # dense_groups(): min(kThreads, scratch cap / slice), spgemm.hip:582
VALIDATE_GRID = 2048                 # validate(), spgemm.hip:640; kValidateGrid, transpose.hip:31
VALIDATE_ITEMS = VALIDATE_GRID * THREADS          # 524 288: the first work item of a second trip
LANES = (1, 2, 4, 8, 16, 32, 64)
SENTINEL = 0x7FC0DEAD                # NaN bits no product here has


# ---- the launch arithmetic, restated --------------------------------------------------------------------------------
def pick_lanes(nnz, rows):
    """pick_lanes_per_row (kernels.hip:467) of the fp32 mean lanes_for (spgemm.hip:495) hands it: lanes double while
    lanes * 4 < mean"""
    mean = np.float32(nnz) / np.float32(max(rows, 1))
    lanes = 1
    while lanes < 64 and lanes * 4 < mean:
        lanes <<= 1
    return lanes


def class_of(key, forced=0):
    """class_of, spgemm.hip:42"""
    if key <= 0:
        return 0
    c = 1
    while c < CLASSES and key > CAPS[c - 1]:
        c += 1
    return forced if 1 <= forced <= CLASSES and forced > c else c


def tables(cls, lanes, symbolic):
    """launch_tables, spgemm.hip:561-568"""
    if cls == CLASSES - 1:
        return 1
    table_bytes = SLOTS[cls - 1] * (4 if symbolic else 8)
    return max(1, min(THREADS // lanes, TABLE_BUDGET // table_bytes))


def workgroup_threads(cls, lanes, symbolic):
    return THREADS if cls == CLASSES - 1 else tables(cls, lanes, symbolic) * lanes


def table_grid(count, cls, lanes, symbolic):
    return min(MAX_GRID, -(-count // tables(cls, lanes, symbolic)))


def trips(count, per_trip):
    return -(-count // per_trip)


def histogram(keys, forced=0):
    """the eight counters of SpGEMMResult for rows with these keys"""
    keys = np.asarray(keys, np.int64)
    cls = np.where(keys > 0, 1 + np.searchsorted(CAPS, keys, side="left"), 0)
    if 1 <= forced <= CLASSES:
        cls = np.where(cls > 0, np.maximum(cls, forced), 0)
    return np.bincount(cls, minlength=8).tolist()


# ---- what the result reports, from numpy ----------------------------------------------------------------------------
def row_lengths(rp):
    return np.diff(np.asarray(rp, np.int64))


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), row_lengths(rp))


def row_products(a, b):
    """per row of A the sum of the lengths of the B rows it names, int64"""
    arp = np.asarray(a[0], np.int64)
    out = np.zeros(arp.size - 1, np.int64)
    if a[1].size:
        np.add.at(out, rows_of(arp), row_lengths(b[0])[a[1]])
    return out


def expected_fields(a, b, c_rp, n, forced=0):
    products, distinct = row_products(a, b), row_lengths(c_rp)
    return {"products": int(products.sum()), "max_row_products": int(products.max(initial=0)),
            "nnz": int(distinct.sum()), "max_row_nnz": int(distinct.max(initial=0)),
            "symbolic_rows": histogram(np.minimum(products, n), forced), "numeric_rows": histogram(distinct, forced)}


def tile_rows(period, m):
    """rows i of the result = row i % P of `period` (P rows), for m rows"""
    rp, ci, va = period
    p = rp.size - 1
    full, rest = divmod(m, p)
    lengths = np.concatenate([np.tile(row_lengths(rp), full), row_lengths(rp)[:rest]])
    out_rp = np.zeros(m + 1, np.int64)
    np.cumsum(lengths, out=out_rp[1:])
    return (out_rp.astype(np.int32), np.concatenate([np.tile(ci, full), ci[:rp[rest]]]).astype(np.int32),
            np.concatenate([np.tile(va, full), va[:rp[rest]]]).astype(np.float32))


def scatter_rows(compact, at, m):
    """the m-row matrix whose rows `at` (ascending) are the rows of `compact` and whose other rows are empty"""
    rp, ci, va = compact
    lengths = np.zeros(m, np.int64)
    lengths[at] = row_lengths(rp)
    out_rp = np.zeros(m + 1, np.int64)
    np.cumsum(lengths, out=out_rp[1:])
    return out_rp.astype(np.int32), ci, va


def other_values(va):
    """the values the values-only pass is handed: every one different from before"""
    return (np.asarray(va, np.float32) * np.float32(0.5) + np.float32(0.125)).astype(np.float32)


def _entries(cols, vals):
    return [(int(c), float(v)) for c, v in zip(cols, vals)]


# ---- A: every (class, lanes) geometry -------------------------------------------------------------------------------
GEOMETRY_LENGTHS = sorted({0} | {v for L in LANES for v in (L - 1, L, L + 1, 2 * L + 1)})     # 0 .. 129, 19 lengths
GEOMETRY_N = 1003                    # no multiple of 32: the dense class's last map word is partial


def geometry_case():
    """335 rows.  B: for every length in GEOMETRY_LENGTHS two rows that share half their columns.  A, unsorted and with
    repeats: every B row alone, every overlapping pair as [second, first, second], random short rows of at most 16
    products (class 1 by themselves; more than 256 of them), random rows of 17 .. 68 products, empty rows and rows
    that name only B's empty rows; in random order."""
    rng = np.random.default_rng(41)
    n = GEOMETRY_N
    b_rows = []
    for length in GEOMETRY_LENGTHS:
        ends = [0, n - 1] if length in (3, 129) else []
        first = np.sort(np.concatenate([ends, 1 + rng.choice(n - 2, size=length - len(ends), replace=False)])).astype(int)
        shared = first[::2]
        rest = np.setdiff1d(np.arange(n), first)
        second = np.sort(np.concatenate([shared, rng.choice(rest, size=length - shared.size, replace=False)]))
        for cols in (first, second):
            b_rows.append(_entries(cols, rng.uniform(-4, 4, cols.size).astype(np.float32)))
    k = len(b_rows)
    length_of = [len(r) for r in b_rows]
    picks = [[r] for r in range(k)] + [[2 * j + 1, 2 * j, 2 * j + 1] for j in range(len(GEOMETRY_LENGTHS))]
    picks += [[] for _ in range(12)]
    short = [r for r in range(k) if length_of[r] <= 5]
    for _ in range(236):                                  # at most 16 products
        row, total = [], 0
        for r in rng.choice(short, size=int(rng.integers(1, 6))).tolist():
            if total + length_of[r] <= 16:
                row.append(r)
                total += length_of[r]
        if row and rng.random() < 0.4 and total + length_of[row[0]] <= 16:
            row.append(row[0])                            # a repeated entry
        picks.append(row)
    medium = [r for r in range(k) if length_of[r] <= 17]
    for _ in range(30):
        row = rng.choice(medium, size=int(rng.integers(2, 5))).tolist()
        picks.append(row + [row[0]])
    order = rng.permutation(len(picks))
    a_rows = [[(r, float(np.float32(rng.uniform(-4, 4)))) for r in picks[i]] for i in order]
    a, b = sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows)
    return {"m": len(a_rows), "k": k, "n": n, "a": a, "b": b, "a2": (a[0], a[1], other_values(a[2]))}


# ---- B: second trips of the table and dense kernels -------------------------------------------------------------------
TRIP_ROWS = 4 * MAX_GRID + 7         # 16 391: at 64 lanes, four tables a workgroup, 4096 workgroups, then 7 rows more
TRIP_PERIOD = 37                     # 16 384 % 37 = 30: a second-trip row is another period row than 16 384 above it
TRIP_N = (5003, 8300)                # n % 32 != 0; 157 map words (fewer than 256 threads) and 260 (a second round)


def trip_case(n):
    """16 391 non-empty rows of at most 16 products: a period of 37 rows of A (unsorted, repeats) over a fixed B of 24
    rows of 1 .. 6 entries, whose columns lie at both ends of [0, n), around the borders of the map words and, with
    n > 8192, on both sides of column 8192."""
    rng = np.random.default_rng(43)
    k = 24
    pool = [0, 1, 31, 32, 33, 63, 64, n // 2, n - 33, n - 2, n - 1] + rng.integers(0, n, 20).tolist()
    if n > 8192:
        pool += [8190, 8191, 8192, 8193, 8224]
    pool = np.unique(pool)
    b_rows = []
    for r in range(k):
        cols = np.sort(rng.choice(pool, size=1 + r % 6, replace=False))
        b_rows.append(_entries(cols, rng.uniform(-2, 2, cols.size).astype(np.float32)))
    a_rows = []
    while len(a_rows) < TRIP_PERIOD:
        row, total = [], 0
        for r in rng.integers(0, k, size=int(rng.integers(1, 5))).tolist():
            if total + len(b_rows[r]) <= 16:
                row.append(r)
                total += len(b_rows[r])
        if len(row) >= 2 and total + len(b_rows[row[0]]) <= 16:
            row.append(row[0])
        a_rows.append([(r, float(np.float32(rng.uniform(-2, 2)))) for r in row])
    period, b = sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows)
    a = tile_rows(period, TRIP_ROWS)
    period2 = (period[0], period[1], other_values(period[2]))
    return {"m": TRIP_ROWS, "k": k, "n": n, "a": a, "b": b, "period": period, "period2": period2,
            "a2": tile_rows(period2, TRIP_ROWS)}


def trip_reference(case, which="period"):
    """the expected C: the period's product by the definition, tiled"""
    p = case[which]
    return tile_rows(sc.product_loop(p[0].size - 1, case["n"], p, case["b"]), case["m"])


# ---- C: the products kernel at 64 lanes per row of A ------------------------------------------------------------------
PRODUCTS_ROWS = 4 * MAX_GRID + 5     # 16 389: four rows a workgroup at 64 lanes, 4096 workgroups, then 5 rows more
PRODUCTS_LONG_ROW = PRODUCTS_ROWS - 3


def products_case():
    """A: 16 389 rows of 124 .. 138 entries (mean above 128: 64 lanes per row) and one of 400 in the second trip, small
    integer values; B: 50 rows of one or two entries over 4 columns, small integer values."""
    rng = np.random.default_rng(47)
    m, k, n = PRODUCTS_ROWS, 50, 4
    b_rows = []
    for r in range(k):                                    # even rows one entry, odd rows two; every column as often
        cols = sorted({(r // 2) % n, (r // 2 + 1) % n}) if r % 2 else [(r // 2) % n]
        b_rows.append(_entries(cols, rng.integers(1, 4, len(cols)) * rng.choice([-1, 1], len(cols))))
    b = sc.csr_from_rows(b_rows)
    lengths = 124 + (np.arange(m) * 7) % 15
    lengths[PRODUCTS_LONG_ROW] = 400
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lengths, out=rp[1:])
    nnz = int(rp[-1])
    ci = rng.integers(0, k, nnz).astype(np.int32)
    ci[rp[PRODUCTS_LONG_ROW]:rp[PRODUCTS_LONG_ROW + 1]] = 1 + 2 * rng.integers(0, k // 2, 400)      # two-entry rows only
    va = (rng.integers(1, 3, nnz) * rng.choice([-1, 1], nnz)).astype(np.float32)
    return {"m": m, "k": k, "n": n, "a": (rp.astype(np.int32), ci, va), "b": b}


def integer_product(m, k, n, a, b):
    """(C, bound): the product of small-integer matrices from int64 arithmetic, and the largest sum of |a| |b| that any
    output column sees.  With bound < 2^24 every partial sum in any order is an integer fp32 holds, so the fp32 product
    is this one whatever the order (a sum that cancels is +0.0: the accumulator starts at +0.0 and x + -x = +0.0)."""
    assert np.array_equal(a[2], np.rint(a[2])) and np.array_equal(b[2], np.rint(b[2]))
    keys = rows_of(a[0]) * k + a[1]
    w_sum = np.rint(np.bincount(keys, weights=a[2].astype(np.float64), minlength=m * k)).astype(np.int64).reshape(m, k)
    w_abs = np.rint(np.bincount(keys, weights=np.abs(a[2]).astype(np.float64), minlength=m * k)).astype(np.int64)
    w_cnt = np.bincount(keys, minlength=m * k).reshape(m, k)
    dense_b = np.zeros((k, n), np.int64)
    has_b = np.zeros((k, n), np.int64)
    dense_b[rows_of(b[0]), b[1]] = b[2].astype(np.int64)
    has_b[rows_of(b[0]), b[1]] = 1
    value = w_sum @ dense_b
    pattern = ((w_cnt > 0).astype(np.int64) @ has_b) > 0
    bound = int((w_abs.reshape(m, k) @ np.abs(dense_b)).max(initial=0))
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(pattern.sum(axis=1), out=rp[1:])
    c = (rp.astype(np.int32), np.nonzero(pattern)[1].astype(np.int32), value[pattern].astype(np.float32))
    return c, bound


# ---- D: the classify kernel's own flag, from workgroup 4097 -----------------------------------------------------------
CLASSIFY_ROWS = MAX_GRID * THREADS + 300          # 1 048 876: 4098 workgroups of spgemm_classify_kernel


def classify_case():
    """Almost all rows empty; 40 non-empty rows of 1 .. 3 entries spread over the matrix, among them rows 0, 1 048 575,
    1 048 576, the first row of workgroup 4097 and row m - 1.  Row m - 1 holds one entry that names B's one-entry row,
    so the last row of C holds one entry; row m - 9 names B's empty row only (entries of A, no products)."""
    rng = np.random.default_rng(53)
    m, k, n = CLASSIFY_ROWS, 16, 40
    b_rows = [[]]
    for r in range(1, k):
        cols = np.sort(rng.choice(n, size=1 + (r - 1) % 4, replace=False))
        b_rows.append(_entries(cols, rng.uniform(-2, 2, cols.size).astype(np.float32)))
    fixed = [0, 255, 256, MAX_GRID * THREADS - 1, MAX_GRID * THREADS, (MAX_GRID + 1) * THREADS, m - 9, m - 2, m - 1]
    at = np.unique(np.concatenate([fixed, rng.integers(0, m, 40 - len(fixed))]))
    a_rows = []
    for i in at.tolist():
        if i == m - 1:
            row = [1]
        elif i == m - 9:
            row = [0]
        else:
            row = rng.integers(1, k, size=int(rng.integers(1, 4))).tolist()
        a_rows.append([(r, float(np.float32(rng.uniform(-2, 2)))) for r in row])
    compact, b = sc.csr_from_rows(a_rows), sc.csr_from_rows(b_rows)
    return {"m": m, "k": k, "n": n, "at": at, "compact": compact, "a": scatter_rows(compact, at, m), "b": b}


def classify_reference(case):
    c = sc.product_loop(case["at"].size, case["n"], case["compact"], case["b"])
    return scatter_rows(c, case["at"], case["m"])


# ---- E: spgemm_validate_kernel past its first trip --------------------------------------------------------------------
SCALED_ROWS = (VALIDATE_ITEMS + 600) // 8         # 65 611 rows of 8 entries: 524 888 entries


def scaled_rows_case():
    """B: 65 611 rows of 8 strictly ascending columns out of 64 (524 888 entries); A: one entry per row, A[i, i].  Every
    output column gets one product, so C[i, :] = fl(+0.0 + fl(a_i * B[i, :])) in any order."""
    rng = np.random.default_rng(59)
    rows, n = SCALED_ROWS, 64
    cols = np.sort(rng.permuted(np.tile(np.arange(n, dtype=np.int32), (rows, 1)), axis=1)[:, :8], axis=1)
    b = (np.arange(rows + 1, dtype=np.int32) * 8, cols.reshape(-1).copy(),
         rng.uniform(-2, 2, rows * 8).astype(np.float32))
    a = (np.arange(rows + 1, dtype=np.int32), np.arange(rows, dtype=np.int32),
         rng.uniform(-2, 2, rows).astype(np.float32))
    return {"m": rows, "k": rows, "n": n, "a": a, "b": b}


def scaled_rows_reference(case):
    a, b = case["a"], case["b"]
    return b[0].copy(), b[1].copy(), (np.float32(0.0) + np.repeat(a[2], 8) * b[2]).astype(np.float32)


def items_that_see(rp, ci, nnz, limit, ascending):
    """the work items of matrix_bad (spgemm.hip:60) that find something wrong"""
    rows = rp.size - 1
    r = np.asarray(rp, np.int64)
    c = np.asarray(ci[:nnz], np.int64)
    bad = set(np.flatnonzero(r[:-1] > r[1:]).tolist())
    if r[0] != 0:
        bad.add(0)
    if r[rows] != nnz:
        bad.add(rows)
    bad.update(np.flatnonzero((c < 0) | (c >= limit)).tolist())
    if ascending:
        i = np.flatnonzero(c[1:] <= c[:-1]) + 1
        bad.update(i[~np.isin(i, r)].tolist())              # legal only where entry i starts a row
    return sorted(bad)


def column_defects(ci, limit, ascending):
    """name -> the column array with its last entry malformed"""
    out = {"the last column equals the limit": limit, "the last column is negative": -1}
    if ascending:
        out = {"an equal adjacent pair at the end of the last row": int(ci[-2]),
               "a descending pair at the end of the last row": int(ci[-2]) - 1,
               "the last column equals num_cols": limit}
    made = {}
    for name, value in out.items():
        bad = ci.copy()
        bad[-1] = value
        made[name] = bad
    return made


# ---- F: transpose_validate_kernel past its first trip -----------------------------------------------------------------
TRANSPOSE_NNZ = VALIDATE_ITEMS + 600
TRANSPOSE_COLS = 70_000
TRANSPOSE_C0 = 5
TRANSPOSE_AT = {8: VALIDATE_ITEMS + 100, 16: VALIDATE_ITEMS + 333}        # bit -> the entry that differs in it alone
TRANSPOSE_VARIANTS = {"bits 8 and 16": (8, 16), "bit 8 alone": (8,), "bit 16 alone": (16,)}


def transpose_case(bits):
    """1200 rows (one long, then rows of three: the second trip spans 200 rows), 524 888 entries, every column 5 but
    for one entry per bit in `bits`, in the second trip"""
    rng = np.random.default_rng(61)
    rows, nnz = 1200, TRANSPOSE_NNZ
    lengths = np.full(rows, 3, np.int64)
    lengths[0] = nnz - 3 * (rows - 1)
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(lengths, out=rp[1:])
    ci = np.full(nnz, TRANSPOSE_C0, np.int32)
    for bit in bits:
        ci[TRANSPOSE_AT[bit]] = TRANSPOSE_C0 ^ (1 << bit)
    return rows, TRANSPOSE_COLS, (rp.astype(np.int32), ci, rng.uniform(-2, 2, nnz).astype(np.float32))


def radix_digits(ci):
    """the 8-bit digits in which some column differs from the first: the passes transpose_build runs"""
    diff = int(np.bitwise_or.reduce(np.asarray(ci, np.int64) ^ int(ci[0])))
    return [d for d in range(4) if (diff >> (8 * d)) & 255]
