"""Generators and numpy references for the edge tests of the build layer (csrc/csr_build.hip):
tests/test_build_edge_cases_host.py proves what each case is named for, tests/test_gpu_build_edges.py runs them.

numpy only; the library is never imported here.  A matrix is (row_ptrs int32, cols int32, vals float32).

* edge_profile: row lengths that make a wrong scan visible (a carry from the wrong tile, a lost carry, a lost total).
* scan_levels / scan_sums / scan_launches: device_scan_levels, device_scan_sums, device_scan_launches restated.
* short_rows_from, spread_columns: matrices with given row lengths.
* np_add_structure, np_permute_rows, np_product_structure, np_transpose, np_coo_sum_structure: the structure of a
  builder's result from cumsum, repeat, unique and a stable argsort alone.
* ROW_OF_SHAPES: explicit row-length lists around the 256 entries one workgroup of expand_rows_kernel takes.
* validate_matrix / validate_defects: the two regimes of the structure check and one defect per run.
A plain module, not a conftest."""
import numpy as np

from spgemm_cases import random_csr

TILE = 4096            # kScanTile: elements per workgroup of the scan
GROUP = 256            # kThreads: entries per workgroup of expand_rows_kernel, work items per workgroup elsewhere
SPRINKLE = 4099        # coprime to TILE
VALIDATE_ITEMS = 2048 * GROUP      # capped_grid's 2048 workgroups: work item 524 288 is the first strided one
IOTA_ITEMS = 1024 * GROUP          # vec_grid's 1024 workgroups
SEGMENTS = 6           # kSegments of spgemm.hip: its class scan has SEGMENTS * m + 1 elements

SCAN_ROWS = (4094, 4095, 4096, 8191, 8192, 12288)      # rows + 1 = 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1
THIRD_LEVEL_ROWS = (TILE * TILE - 1, TILE * TILE)       # rows + 1 = 4096^2 (two levels), 4096^2 + 1 (three)
SPGEMM_ROWS = (682, 683, 1365, 1366, 4095, 4096)        # 6 m + 1 = 4093, 4099, 8191, 8197; m + 1 = 4096, 4097
SPGEMM_THIRD_LEVEL_ROWS = (2_796_202, 2_796_203)        # 6 m + 1 = 16 777 213, 16 777 219
FSAI_ROWS = (4095, 4096, 8192)
MIS2_ROWS = (4095, 4096, 8192)
COO_TRIPLETS = (4095, 4096, 8191, 8192)
TRANSPOSE_NNZ = (16 * TILE, 16 * TILE + 1, 17 * TILE + 3)      # 16, 17, 18 tiles of 4096 entries: 256 counts each


# ---- the scan's geometry, restated ------------------------------------------------------------------------------
def scan_levels(n, tile=TILE):
    sizes = [int(n)]
    while sizes[-1] > 1:
        sizes.append((sizes[-1] + tile - 1) // tile)
    return sizes


def scan_sums(levels):
    return 1 + sum(levels[1:])


def scan_launches(levels):
    """a tile kernel per level below the top, an add kernel for all but the last of them: 1, 3, 5"""
    return max(1, 2 * len(levels) - 3)


def scan_depth(n, tile=TILE):
    """levels that run a tile kernel: 1 up to one tile, 2 up to tile^2, 3 beyond"""
    return max(1, len(scan_levels(n, tile)) - 1)


# ---- row lengths ------------------------------------------------------------------------------------------------
def border_rows(rows, tile=TILE):
    """(a): rows 0, k tile - 2, k tile - 1, k tile, k tile + 1 for every multiple k tile <= rows, and the last row"""
    k = np.arange(1, rows // tile + 1, dtype=np.int64) * tile
    at = np.concatenate([[0, rows - 1], k - 2, k - 1, k, k + 1])
    return np.unique(at[(at >= 0) & (at < rows)])


def empty_tile(rows, tile=TILE):
    """(b): the tile left empty, or None where there are fewer than three whole tiles of rows.  It is the second one:
    sums[1] = 0 between two other totals.  The positions of (a) and (d) inside it are empty too."""
    return 1 if rows >= 3 * tile else None


def sprinkle_rows(rows):
    """(d): every 4099th row"""
    return np.arange(0, rows, SPRINKLE, dtype=np.int64)


def tile_totals(lengths, tile=TILE):
    """the totals of the tiles of the scanned array: the lengths and one 0 behind them"""
    padded = np.zeros(-(-(lengths.size + 1) // tile) * tile, np.int64)
    padded[:lengths.size] = lengths
    return padded.reshape(-1, tile).sum(axis=1)


def edge_profile(rows, tile=TILE, seed=0):
    """Row lengths 0 .. 3 with
    (a) a non-zero at border_rows(rows),
    (b) one whole tile of empty rows with a non-empty tile behind it (rows >= 3 tile; see empty_tile),
    (c) every tile total different from both neighbours',
    (d) a non-zero at every 4099th row, and with tile^2 rows or more at every in-tile offset somewhere.
    Everything else is empty: the rows matter, not the entries."""
    rng = np.random.default_rng(seed)
    lengths = np.zeros(rows, np.int32)
    fixed = np.union1d(border_rows(rows, tile), sprinkle_rows(rows))
    lengths[fixed] = rng.integers(1, 4, fixed.size)
    hole = empty_tile(rows, tile)
    if hole is not None:
        lengths[hole * tile:(hole + 1) * tile] = 0
    if rows >= tile * tile:                               # (d): the offsets the stride has not reached, in tiles 3 .. 7
        missing = np.setdiff1d(np.arange(tile), np.flatnonzero(lengths) % tile)
        extra = missing + tile * (3 + missing % 5)
        lengths[extra] = rng.integers(1, 4, extra.size)
    # (c): where a tile's total equals the one before it, one more non-zero at its third row (or another value there)
    totals = tile_totals(lengths, tile)
    for b in range(1, totals.size):
        at = b * tile + 2
        if totals[b] != totals[b - 1] or b == hole or at >= rows:
            continue
        new = next(v for v in (1, 2, 3) if v != lengths[at])
        totals[b] += new - lengths[at]
        lengths[at] = new
    return lengths


def row_ptrs_of(lengths):
    """the cumsum in int64, cast after checking that it fits"""
    rp = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=rp[1:])
    assert rp[-1] <= np.iinfo(np.int32).max
    return rp.astype(np.int32)


def rows_of(rp):
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int32), np.diff(rp))


def short_rows_from(lengths, seed, cols=16):
    """A matrix with the given row lengths (0 .. 3), strictly ascending columns below `cols` (>= 12): two of these from
    different seeds share some columns and miss others."""
    assert cols >= 12 and (lengths.size == 0 or lengths.max() <= 3)
    rng = np.random.default_rng(seed)
    rp = row_ptrs_of(lengths)
    filled = np.flatnonzero(lengths)
    steps = rng.integers(1, 5, size=(filled.size, 3))
    steps[:, 0] -= 1
    ascending = np.cumsum(steps, axis=1)
    keep = np.arange(3)[None, :] < lengths[filled][:, None]
    ci = ascending[keep].astype(np.int32)
    return rp, ci, rng.uniform(-2, 2, size=ci.size).astype(np.float32)


def spread_columns(lengths, cols, seed):
    """A matrix with the given row lengths and columns drawn from the whole of [0, cols), any order, repeats allowed"""
    rng = np.random.default_rng(seed)
    rp = row_ptrs_of(np.asarray(lengths, np.int32))
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32)
    if nnz >= 2:
        ci[0], ci[-1] = 0, cols - 1
    return rp, ci, rng.uniform(-2, 2, nnz).astype(np.float32)


# ---- numpy references of the structure --------------------------------------------------------------------------
def np_add_structure(rows, cols, a, b):
    """(row_ptrs, cols) of A + B with ascending rows: the sorted union of the keys row * cols + col"""
    keys = np.union1d(rows_of(a[0]).astype(np.int64) * cols + a[1], rows_of(b[0]).astype(np.int64) * cols + b[1])
    rp = row_ptrs_of(np.bincount(keys // cols, minlength=rows).astype(np.int64)) if rows else np.zeros(1, np.int32)
    return rp, (keys % cols).astype(np.int32)


def np_permute_rows(a, row_perm):
    """B's arrays for row i of B = row row_perm[i] of A, the columns (ascending in A, not renamed) as they are"""
    rp, ci, va = a
    lengths = np.diff(np.asarray(rp, np.int64))[row_perm]
    inverse = np.empty(row_perm.size, np.int64)
    inverse[row_perm] = np.arange(row_perm.size)
    order = np.argsort(inverse[rows_of(rp)], kind="stable")
    return row_ptrs_of(lengths), ci[order], va[order]


def np_product_structure(m, n, a, b):
    """(row_ptrs, cols) of A B for n <= 64: per row of A the OR of the column sets of the B rows it names"""
    assert n <= 64
    brp = np.asarray(b[0], np.int64)
    sets = np.zeros(brp.size - 1, np.uint64)
    np.bitwise_or.at(sets, rows_of(brp), np.uint64(1) << b[1].astype(np.uint64))
    arp = np.asarray(a[0], np.int64)
    filled = np.flatnonzero(np.diff(arp))
    row_sets = np.zeros(m, np.uint64)
    if filled.size:
        row_sets[filled] = np.bitwise_or.reduceat(sets[a[1]], arp[:-1][filled])
    has = (row_sets[filled][:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)
    lengths = np.zeros(m, np.int64)
    lengths[filled] = has.sum(axis=1)
    return row_ptrs_of(lengths), np.nonzero(has)[1].astype(np.int32)


def np_transpose(rows, cols, rp, ci, va):
    """the stable argsort by column"""
    order = np.argsort(ci, kind="stable")
    return row_ptrs_of(np.bincount(ci, minlength=cols).astype(np.int64)), rows_of(rp)[order], va[order]


def np_coo_sum_structure(rows, cols, r, c):
    """(row_ptrs, cols) of the COO_SUM assembly: the distinct (row, col) pairs in order"""
    keys = np.unique(np.asarray(r, np.int64) * cols + c)
    return row_ptrs_of(np.bincount(keys // cols, minlength=rows).astype(np.int64)), (keys % cols).astype(np.int32)


# ---- the cases of the scan's callers ------------------------------------------------------------------------------
def add_pair(rows, cols=16):
    """A and B of csr_add: two edge profiles of different seeds, some columns shared"""
    return short_rows_from(edge_profile(rows, seed=1), 11, cols), short_rows_from(edge_profile(rows, seed=2), 12, cols)


def product_pair(m, k=16, n=64):
    """A (m x k) and B (k x n, spgemm_cases.random_csr) of spgemm_csr.  B's rows hold about ten entries, so one to three
    of them bound a row of C by 0 (no products), by 16 or less (the first accumulator class) or by more (the second).
    A's row lengths are an edge profile; up to four tiles of rows four in ten of its empty rows are filled as well, so
    that each class has rows on both sides of the tile borders of the class scan (every row is a 1 in one of its six
    segments of m flags)."""
    lengths = edge_profile(m, seed=3)
    if m <= 4 * TILE:
        rng = np.random.default_rng(6)
        lengths = np.where((lengths == 0) & (rng.random(m) < 0.4), rng.integers(1, 4, m), lengths).astype(np.int32)
    a = short_rows_from(lengths, 13, k)
    return a, random_csr(np.random.default_rng(5), k, n, 0.15)


def product_bounds(a, b):
    """per row of A the sum of the lengths of the B rows it names: what chooses the accumulator class"""
    arp = np.asarray(a[0], np.int64)
    bound = np.zeros(arp.size - 1, np.int64)
    filled = np.flatnonzero(np.diff(arp))
    if filled.size:
        bound[filled] = np.add.reduceat(np.diff(np.asarray(b[0], np.int64))[a[1]], arp[:-1][filled])
    return bound


def coo_triplets(count, rows=700, cols=40, seed=7):
    """`count` triplets in random order, about a third of them repeats of an earlier (row, col)"""
    rng = np.random.default_rng(seed + count)
    distinct = count - count // 3
    keys = rng.choice(rows * cols, size=distinct, replace=False)
    keys = np.concatenate([keys, rng.choice(keys, size=count - distinct)])
    keys = keys[rng.permutation(count)]
    return (keys // cols).astype(np.int32), (keys % cols).astype(np.int32), rng.uniform(-2, 2, count).astype(np.float32)


def transpose_case(nnz, passes):
    """(rows, cols, matrix) with nnz entries and columns spread over `passes` radix digits of 8 bits (0: all equal)"""
    cols = {0: 1, 1: 200, 2: 60_000, 3: 70_000}[passes]
    rows = nnz // 2 + 5
    lengths = np.zeros(rows, np.int64)
    lengths[::2][:nnz // 2] = 2
    lengths[1] = nnz - int(lengths.sum())
    return rows, cols, spread_columns(lengths, cols, nnz + passes)


def radix_passes(cols):
    return 0 if cols <= 1 else -(-int(cols - 1).bit_length() // 8)


# ---- row_of at the workgroup edges --------------------------------------------------------------------------------
def _row_of_shapes():
    shapes = {}
    for nnz in (1, 255, 256, 257, 511, 512, 513):
        shapes[f"{nnz} in one row"] = [nnz]
        shapes[f"{nnz} rows of one"] = [1] * nnz
    for end in (255, 256, 257):
        shapes[f"a row ends on entry {end}"] = [end, 3, 300]
    shapes["a row of 1000 between rows of one"] = [1, 1000, 1]
    shapes["600 empty rows inside one workgroup"] = [50, 51] + [0] * 600 + [7, 100]
    shapes["300 empty rows at either end"] = [0] * 300 + [3, 0, 260, 1] + [0] * 300
    shapes["one row"] = [5]
    shapes["rows that start at multiples of 256"] = [256, 0, 0, 512, 0, 256, 256, 0]
    return {name: np.asarray(l, np.int32) for name, l in shapes.items()}


ROW_OF_SHAPES = _row_of_shapes()


def row_ends(lengths):
    """the entry behind each non-empty row's last one"""
    ends = np.cumsum(np.asarray(lengths, np.int64))
    return ends[np.asarray(lengths) > 0]


# ---- the structure check ------------------------------------------------------------------------------------------
VALIDATE_ROWS, VALIDATE_COLS = 600_000, 1000


def validate_matrix(regime):
    """600 000 x 1000; "entries" has about 700 000 entries (nnz > rows + 1), "rows" about 1000 (nnz < rows + 1)"""
    lengths = edge_profile(VALIDATE_ROWS, seed=9)
    if regime == "entries":
        rng = np.random.default_rng(10)
        lengths[rng.random(VALIDATE_ROWS) < 0.58] += 2
    else:
        filled = np.flatnonzero(lengths)
        keep = filled[np.arange(filled.size) % 3 != 2]
        thin = np.zeros_like(lengths)
        thin[keep] = lengths[keep]
        lengths = thin
        lengths[[0, VALIDATE_ITEMS - 1, VALIDATE_ITEMS, VALIDATE_ROWS - 2, VALIDATE_ROWS - 1]] = 1
    rp = row_ptrs_of(lengths)
    nnz = int(rp[-1])
    rng = np.random.default_rng(11)
    return rp, rng.integers(0, VALIDATE_COLS, nnz).astype(np.int32), np.ones(nnz, np.float32)


def validate_defects(rp, ci, cols=VALIDATE_COLS):
    """name -> (array, index, value): one malformed word each.  Column defects where the matrix has that entry."""
    rows, nnz = rp.size - 1, ci.size
    out = {}
    for at in (0, VALIDATE_ITEMS, nnz - 1):
        if at < nnz:
            out[f"column -1 at entry {at}"] = ("cols", at, -1)
            out[f"column = cols at entry {at}"] = ("cols", at, cols)
    out["row_ptrs[0] = 1"] = ("row_ptrs", 0, 1)
    out["row_ptrs[rows] = nnz - 1"] = ("row_ptrs", rows, nnz - 1)
    out["row_ptrs[rows] = nnz + 1"] = ("row_ptrs", rows, nnz + 1)
    for row in (1, VALIDATE_ITEMS, rows - 1):
        # row_ptrs[row] > row_ptrs[row + 1]: the decrease is seen by work item `row` and by no other
        out[f"a decrease at row {row}"] = ("row_ptrs", row, int(rp[row + 1]) + 1)
    return out


# the two defects every other door of the check is handed: only a strided trip of the check sees them
DOOR_DEFECTS = (f"column -1 at entry {VALIDATE_ITEMS}", f"a decrease at row {VALIDATE_ITEMS}")


def with_defect(rp, ci, defect):
    array, index, value = defect
    rp, ci = rp.copy(), ci.copy()
    (rp if array == "row_ptrs" else ci)[index] = value
    return rp, ci


def is_valid(rp, ci, cols, nnz):
    """the rule of csr_validate_kernel"""
    return bool(rp[0] == 0 and rp[-1] == nnz and np.all(np.diff(rp.astype(np.int64)) >= 0) and
                (ci.size == 0 or (ci.min() >= 0 and ci.max() < cols)))


def items_that_see(rp, ci, cols, nnz):
    """the work items of csr_validate_kernel that find something wrong"""
    rows = rp.size - 1
    r = rp.astype(np.int64)
    bad = set(np.flatnonzero(r[:-1] > r[1:]).tolist())
    if r[0] != 0:
        bad.add(0)
    if r[rows] != nnz:
        bad.add(rows)
    bad.update(np.flatnonzero((ci < 0) | (ci >= cols)).tolist())
    return sorted(bad)
