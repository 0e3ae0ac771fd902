"""Exact-arithmetic test data: matrices and vectors of small integers stored as float32.

When, for every row, sum_j |a_ij| * |x_j| < 2^24, every partial sum of the row, taken in any order, fused or
unfused, in fp32 or through fp64, is an integer below 2^24 and therefore exact.  Every summation order then gives the
same bits, so a kernel that reorders a row's sum can be held to BIT EQUALITY with a plain int64 reference: a dropped
reduction step, a gather from a neighbour's entry or a lost carry shows as a wrong integer, not as "rounding".

The module also holds the catalogue of matrices the exact GPU tests run (tests/test_gpu_lane_sweep.py), so that
tests/test_exact_data.py can prove, without a GPU, that each one is exact and lands on the kernel instantiation
its name claims.  A plain module, imported by those tests; everything is built with numpy from fixed seeds."""
import numpy as np

EXACT_LIMIT = 1 << 24
LANES = (1, 2, 4, 8, 16, 32, 64)
MERGE_TILE = 1792        # kMergeTile (csrc/kernels.hip) and kMultiTile (csrc/spmm.hip): merge items per workgroup


# ------------------------------------------------------------------------------------------ the lane rule
def lanes_for(nnz, rows):
    """Restatement of pick_lanes_per_row (csrc/kernels.hip) applied to float(nnz) / rows as its callers compute
    it, in float32: the smallest L in 1..64 with 4 * L >= average, 64 when none is."""
    avg = np.float32(nnz) / np.float32(rows)
    lanes = 1
    while lanes < 64 and np.float32(lanes * 4) < avg:
        lanes <<= 1
    return lanes


# ------------------------------------------------------------------------------------------ exact data
def row_abs_sums(row_ptrs, cols, vals, x):
    """sum_j |a_ij| * |x_j| per row in int64; x is a vector or a (num_cols, k) matrix (then the worst column)."""
    row_ptrs = np.asarray(row_ptrs, np.int64)
    x = np.abs(np.asarray(x).astype(np.int64))
    worst = x if x.ndim == 1 else x.max(axis=1)
    prod = np.abs(np.asarray(vals).astype(np.int64)) * worst[np.asarray(cols)]
    run = np.concatenate([[0], np.cumsum(prod)])
    return run[row_ptrs[1:]] - run[row_ptrs[:-1]]


def check_exact(row_ptrs, cols, vals, x):
    """The condition that makes the data order-independent (module docstring); integers throughout."""
    vals, x = np.asarray(vals), np.asarray(x)
    assert vals.dtype == np.float32 and x.dtype == np.float32
    assert np.array_equal(vals, np.rint(vals)) and np.array_equal(x, np.rint(x))
    sums = row_abs_sums(row_ptrs, cols, vals, x)
    assert sums.size == 0 or int(sums.max()) < EXACT_LIMIT, int(sums.max())


def exact_csr(rng, lens, num_cols, vmax=8, xmax=64):
    """(row_ptrs, cols, vals, x) for the given row lengths: values non-zero integers in [-vmax, vmax], x integers
    in [-xmax, xmax], both float32; columns scattered, unsorted, repeats allowed.  The defaults allow rows of up to
    32 767 entries; longer rows need a smaller vmax / xmax (check_exact fails otherwise)."""
    lens = np.asarray(lens, np.int64)
    row_ptrs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(row_ptrs[-1])
    cols = rng.integers(0, num_cols, size=nnz).astype(np.int32)
    vals = (rng.integers(1, vmax + 1, size=nnz) * rng.choice([-1, 1], size=nnz)).astype(np.float32)
    x = rng.integers(-xmax, xmax + 1, size=num_cols).astype(np.float32)
    check_exact(row_ptrs, cols, vals, x)
    return row_ptrs, cols, vals, x


def exact_x_matrix(rng, num_cols, width, xmax=64):
    """An integer X (num_cols, width) for spmv_csr_multi; check_exact takes it column by column."""
    return rng.integers(-xmax, xmax + 1, size=(num_cols, width)).astype(np.float32)


def exact_reference(row_ptrs, cols, vals, x):
    """y = A x in int64, returned as float32 (exact under check_exact's condition)."""
    row_ptrs = np.asarray(row_ptrs, np.int64)
    prod = np.asarray(vals).astype(np.int64) * np.asarray(x).astype(np.int64)[np.asarray(cols)]
    run = np.concatenate([[0], np.cumsum(prod)])
    y = run[row_ptrs[1:]] - run[row_ptrs[:-1]]
    assert y.size == 0 or int(np.abs(y).max()) < EXACT_LIMIT
    return y.astype(np.float32)


def lens_for_average(rows, avg_num, avg_den, rng):
    """Ragged row lengths whose total is exactly rows * avg_num / avg_den: every 11th row and the last one empty,
    one row (rows // 3) five times the average, the others scattered between 0 and twice the average."""
    assert (rows * avg_num) % avg_den == 0
    total = rows * avg_num // avg_den
    lens = np.zeros(rows, np.int64)
    hub = rows // 3
    free = np.ones(rows, bool)
    free[::11] = False
    free[-1] = False
    free[hub] = False
    if total >= 10:
        lens[hub] = min(total // 2, max(5, 5 * -(-total // rows)))
    share = (total - lens[hub]) / max(int(free.sum()), 1)
    if share >= 1:
        lens[free] = rng.integers(0, int(2 * share) + 1, size=int(free.sum()))
    diff = total - int(lens.sum())
    while diff != 0:            # single entries added to / taken from random free rows until the total is met
        eligible = np.flatnonzero(free if diff > 0 else free & (lens > 0))
        picked = rng.choice(eligible, size=min(abs(diff), eligible.size), replace=False)
        lens[picked] += 1 if diff > 0 else -1
        diff = total - int(lens.sum())
    return lens


# ------------------------------------------------------------------------------------------ lane sweep catalogue
def sweep_counts(rows):
    """[(name, L, nnz)]: per L the top of its range (nnz == 4 L rows; an average of 200 for L = 64) and the
    smallest count above the previous threshold (nnz == 4 (L/2) rows + 1; half an entry per row for L = 1)."""
    out = []
    for L in LANES:
        low = rows // 2 if L == 1 else 2 * L * rows + 1
        top = 200 * rows if L == 64 else 4 * L * rows
        out += [("L%d_low" % L, L, low), ("L%d_top" % L, L, top)]
    return out


SWEEP_ROWS, SWEEP_COLS = 1003, 3001          # 1003 is odd: the last workgroup has idle row slots at every L
LDSX_ROWS = 4099                             # >= 4096 rows; odd, so not a multiple of 1024 / L


def sweep_matrix(name, rows=SWEEP_ROWS, num_cols=SWEEP_COLS):
    """(L, row_ptrs, cols, vals, x) of one lane-sweep case."""
    index, (_, L, nnz) = next((i, c) for i, c in enumerate(sweep_counts(rows)) if c[0] == name)
    rng = np.random.default_rng(1000 * rows + index)
    lens = lens_for_average(rows, nnz, rows, rng)
    return (L,) + exact_csr(rng, lens, num_cols)


def ldsx_cols(index, nnz):
    """Columns of the x-in-LDS case: vector_ldsx_grid (csrc/kernels.hip) wants nnz >= 256 * num_cols.  Even
    cases get a multiple of four (16-byte copy loop without a tail), odd ones do not."""
    cols = min(SWEEP_COLS, nnz // 256)
    if index % 2 == 0:
        return cols - cols % 4 if cols >= 4 else cols
    return cols - 1 if cols % 4 == 0 else cols


def ldsx_matrix(name):
    """(L, num_cols, row_ptrs, cols, vals, x) of one x-in-LDS lane-sweep case."""
    index, (_, L, nnz) = next((i, c) for i, c in enumerate(sweep_counts(LDSX_ROWS)) if c[0] == name)
    num_cols = ldsx_cols(index, nnz)
    rng = np.random.default_rng(7000 + index)
    lens = lens_for_average(LDSX_ROWS, nnz, LDSX_ROWS, rng)
    return (L, num_cols) + exact_csr(rng, lens, num_cols)


SWEEP_NAMES = [c[0] for c in sweep_counts(SWEEP_ROWS)]


# ------------------------------------------------------------------------------------------ merge-path cut points
def _short(rng, count):
    return list(rng.integers(0, 9, size=count))


def _row_ending_at(lens, item):
    """Appends the row whose row-end item is merge item `item` (0-based): the row-end item of row r is item
    row_ptrs[r + 1] + r of the merge list (a row's entries, then its end)."""
    r, before = len(lens), int(sum(lens))
    assert item - r - before >= 0
    return lens + [item - r - before]


def merge_cut_lens(name):
    """Row lengths of the merge-path cases.  Shapes are placed against tiles of MERGE_TILE = 1 792 merge items
    (rows + entries); if the tile size changes, move them."""
    T = MERGE_TILE
    rng = np.random.default_rng(sum(name.encode()))
    if name.startswith("total_"):                   # rows + nnz == the given total
        total = {"total_T-1": T - 1, "total_T": T, "total_T+1": T + 1, "total_2T": 2 * T, "total_2T+1": 2 * T + 1}[name]
        rows = 301
        return list(lens_for_average(rows, total - rows, rows, rng))
    if name.startswith("row_end_"):                 # a row's end is the last item of tile 0 / the one before / tile 1's first
        item = {"row_end_T-2": T - 2, "row_end_T-1": T - 1, "row_end_T": T}[name]
        return _row_ending_at(_short(rng, 150), item) + _short(rng, 400)
    if name == "row_over_four_tiles":               # begins in tile 0, ends in tile 3: tiles 0, 1, 2 carry into it
        return _row_ending_at(_short(rng, 120), 3 * T + T // 2) + _short(rng, 200)
    if name == "two_rows_over_four_tiles":          # the second begins in tile 3 and ends in tile 6
        return _row_ending_at(_row_ending_at(_short(rng, 120), 3 * T + T // 2), 6 * T + T // 2) + _short(rng, 200)
    if name == "empty_run_in_the_middle":
        return _short(rng, 150) + [0] * 2000 + _short(rng, 150)
    if name == "empty_run_at_the_end":
        return _short(rng, 150) + [0] * 2000
    if name == "tile_begins_with_old_row_end":      # tile 2's first item ends a row that began in tile 0
        return _row_ending_at(_short(rng, 100), 2 * T) + _short(rng, 300)
    raise KeyError(name)


MERGE_CUT_NAMES = ["total_T-1", "total_T", "total_T+1", "total_2T", "total_2T+1", "row_end_T-2", "row_end_T-1",
                   "row_end_T", "row_over_four_tiles", "two_rows_over_four_tiles", "empty_run_in_the_middle",
                   "empty_run_at_the_end", "tile_begins_with_old_row_end"]
MERGE_CUT_COLS = 2003


def merge_cut_matrix(name):
    """(row_ptrs, cols, vals, x) of one merge-path case."""
    rng = np.random.default_rng(31 + MERGE_CUT_NAMES.index(name))
    return exact_csr(rng, merge_cut_lens(name), MERGE_CUT_COLS)


# ------------------------------------------------------------------------------------------ integer systems
def _csr_from_triplets(n, rows, cols, vals):
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp.astype(np.int32), cols[order].astype(np.int32), vals[order].astype(np.float32)


def _integer_offdiagonal(rng, n, count, vmax):
    """`count` scattered off-diagonal entries (row, column, non-zero integer in [-vmax, vmax]); rows are drawn, not
    dealt, so row lengths are ragged, and a (row, column) pair may repeat (its entries add up)."""
    r = rng.integers(0, n, size=count)
    c = rng.integers(0, n, size=count)
    c = np.where(c == r, (c + 1) % n, c)
    v = rng.integers(1, vmax + 1, size=count) * rng.choice([-1, 1], size=count)
    return r, c, v


def integer_spd(n, offdiagonal, seed, vmax=3):
    """S + S^T + D as spd.random_spd builds it, in integers: S holds `offdiagonal` entries, D_ii = the row sum of
    |S| + |S^T| plus one, so the matrix is symmetric and strictly diagonally dominant with a positive diagonal, hence
    SPD.  nnz = 2 * offdiagonal + n."""
    rng = np.random.default_rng(seed)
    r, c, v = _integer_offdiagonal(rng, n, offdiagonal, vmax)
    d = np.bincount(r, weights=np.abs(v), minlength=n) + np.bincount(c, weights=np.abs(v), minlength=n) + 1
    diag = np.arange(n)
    return _csr_from_triplets(n, np.concatenate([r, c, diag]), np.concatenate([c, r, diag]),
                              np.concatenate([v, v, d.astype(np.int64)]))


def integer_nonsym(n, offdiagonal, seed, vmax=3):
    """S + D in integers: non-symmetric, strictly row diagonally dominant (D_ii = the row sum of |S| plus one), the
    diagonal entry stored last in its row as nonsym.random_nonsym does.  nnz = offdiagonal + n."""
    rng = np.random.default_rng(seed)
    r, c, v = _integer_offdiagonal(rng, n, offdiagonal, vmax)
    d = np.bincount(r, weights=np.abs(v), minlength=n) + 1
    diag = np.arange(n)
    return _csr_from_triplets(n, np.concatenate([r, diag]), np.concatenate([c, diag]),
                              np.concatenate([v, d.astype(np.int64)]))


def solver_counts():
    """[(name, L, n, nnz)] for the solvers' lane sweep: nnz == 4 L n and nnz == 4 (L/2) n + 1 as for sweep_counts.
    A non-singular matrix stores its n diagonal entries, so the average cannot go below one: L = 1's lower case is
    the diagonal plus one symmetric pair (n + 2).  n is even or odd as the symmetric count 2 |S| + n requires."""
    out = []
    for L in LANES:
        n_low, n_top = 1201, 1202
        low = n_low + 2 if L == 1 else 2 * L * n_low + 1
        top = 200 * n_top if L == 64 else 4 * L * n_top
        out += [("L%d_low" % L, L, n_low, low), ("L%d_top" % L, L, n_top, top)]
    return out


SOLVER_NAMES = [c[0] for c in solver_counts()]


def solver_system(name, symmetric):
    """(L, n, row_ptrs, cols, vals, x_star, b) of one solver case: x_star and b are integer vectors in [-64, 64]
    (b is the right-hand side of the solves from x0 = 0; A x_star is the right-hand side of the exact init test)."""
    index, (_, L, n, nnz) = next((i, c) for i, c in enumerate(solver_counts()) if c[0] == name)
    if symmetric:
        assert (nnz - n) % 2 == 0
        n, rp, ci, va = integer_spd(n, (nnz - n) // 2, seed=50 + index)
    else:
        n, rp, ci, va = integer_nonsym(n, nnz - n, seed=80 + index)
    assert int(rp[-1]) == nnz
    rng = np.random.default_rng(900 + index)
    x_star = rng.integers(-64, 65, size=n).astype(np.float32)
    b = rng.integers(-64, 65, size=n).astype(np.float32)
    b[b == 0] = 1.0
    check_exact(rp, ci, va, x_star)
    check_exact(rp, ci, va, b)
    return L, n, rp, ci, va, x_star, b


# PageRank graphs: k links per row, at the top of each L's range and just above the previous threshold (the links
# into the dangling nodes are removed, which takes a few thousandths off the average: never enough to cross a
# threshold, as tests/test_exact_data.py checks).
PAGERANK_N = 1501
PAGERANK_DANGLING = (3, 700, 1500)
PAGERANK_CASES = [("L%d_%s" % (L, side), L, k) for L in LANES
                  for side, k in (("low", 1 if L == 1 else 2 * L + 1), ("top", 200 if L == 64 else 4 * L))]


def pagerank_graph(spmv, graph, k, seed):
    """test_gpu_pagerank.graph (passed in as `graph`) up to the 64 links per row synth.uniform_csr can draw; beyond
    that the same graph built from synth.stratified_csr (k distinct columns per row), the links into the dangling
    nodes removed and the weights made column-stochastic in the same way."""
    n = PAGERANK_N
    if k <= 64:
        return graph(spmv, n, k, seed, dangling=PAGERANK_DANGLING)
    rp, ci, _ = spmv.synth.stratified_csr(seed, 0, np.full(n, k), n)
    keep = ~np.isin(ci, np.array(PAGERANK_DANGLING, np.int32))
    counts = np.add.reduceat(keep.astype(np.int64), rp[:-1])
    ci = ci[keep]
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return rp, ci, spmv.synth.column_stochastic_values(ci, n)

def ell_cases():
    """(width, rows, row_ptrs, cols, vals, x): widths 1..9 crossed with rows % 4 in 0..3, ragged rows (padding in
    every slab but the first), one row of the full width.  rows % 4 == 0 runs ell_kernel_x4, the others
    ell_kernel_x1; widths 1..9 take both kernels' unrolled-by-four loops through every remainder."""
    for width in range(1, 10):
        for mod in range(4):
            rows = 260 + mod
            rng = np.random.default_rng(100 * width + mod)
            lens = rng.integers(0, width + 1, size=rows)
            lens[rng.integers(0, rows)] = width
            yield (width, rows) + exact_csr(rng, lens, 300)
