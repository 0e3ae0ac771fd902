"""Exact-arithmetic test data: matrices and vectors of small integers stored as float32.

When, for every row, sum_j |a_ij| * |x_j| < 2^24, every partial sum of the row, taken in any order, fused or
unfused, in fp32 or through fp64, is an integer below 2^24 and therefore exact.  Every summation order then gives the
same bits, so a kernel that reorders a row's sum can be held to BIT EQUALITY with a plain int64 reference: a dropped
reduction step, a gather from a neighbour's entry or a lost carry shows as a wrong integer, not as "rounding".

The module also holds the catalogue of matrices the exact GPU tests run (tests/test_gpu_lane_sweep.py), so that
tests/test_exact_data.py can prove, without a GPU, that each one is exact and lands on the kernel instantiation
its name claims.  A plain module, imported by those tests; everything is built with numpy from fixed seeds."""
import math

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


# ------------------------------------------------------------------------------------------ dyadic PageRank
# With n = 2^k nodes, a dyadic damping factor (0.5), every out-degree a power of two (values 2^-j) and the start
# vector 1/n, every quantity of pagerank()'s update r_new = d * (A r) + d * s / n + (1 - d) / n is a dyadic rational.
# While each of them fits float32's 24 bits, every summation order and every rounding gives the same bits, and the
# device result can be held to BIT EQUALITY with integer arithmetic.  The prover below counts the steps for which
# that holds; nothing is assumed.
def dyadic_graph(rng, n, out_degrees, dangling, hubs):
    """(row_ptrs, cols, vals) of an n x n adjacency matrix, n a power of two: column c links to out-degree(c)
    distinct rows, the degree drawn from `out_degrees` (powers of two) and stored as 2^-j in every entry of the
    column (one value per column: the tiled plan folds them); the columns in `dangling` have no entries; `hubs` is
    a list of (row, length): that row is linked from `length` columns; rows with row % 13 == 5 stay empty unless
    they are hubs.  Columns inside a row are distinct and ascending."""
    assert n & (n - 1) == 0 and all(g & (g - 1) == 0 for g in out_degrees)
    deg = rng.choice(np.asarray(out_degrees, np.int64), size=n)
    deg[np.asarray(dangling, np.int64)] = 0
    hub_rows = np.array([h for h, _ in hubs], np.int64)
    allowed = np.ones(n, bool)
    allowed[5::13] = False
    allowed[hub_rows] = False
    perm = rng.permutation(np.flatnonzero(allowed))
    m = perm.size
    assert max(out_degrees) <= m
    first = np.cumsum(deg) - deg
    col_of = np.repeat(np.arange(n, dtype=np.int64), deg)
    within = np.arange(col_of.size, dtype=np.int64) - np.repeat(first, deg)
    row_of = perm[(rng.integers(0, m, size=n)[col_of] + within) % m]          # a window of the permutation: distinct rows
    for k, (hub, length) in enumerate(hubs):                                    # link k of `length` columns goes to the hub
        candidates = np.flatnonzero(deg > k)
        assert candidates.size >= length
        row_of[first[rng.choice(candidates, size=length, replace=False)] + k] = hub
    order = np.lexsort((col_of, row_of))
    ci = col_of[order].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(row_of, minlength=n))]).astype(np.int32)
    va = (1.0 / deg[ci]).astype(np.float32)
    return rp, ci, va


def _fits_float32(v):
    """Whether each integer of v (any common power-of-two scale) has at most 24 significant bits."""
    v = np.abs(np.asarray(v, np.int64))
    return bool(np.all((v >> 24) < (v & -v) + (v == 0)))


def _dyadic_run(rp, ci, va, n, damping, steps):
    """pagerank()'s loop in int64 over a power-of-two quantum.  Yields per step (ranks float32, exact residual
    float64, whether every operation of the step was exact in float32)."""
    k = n.bit_length() - 1
    assert n == 1 << k
    d = float(np.float32(damping)).as_integer_ratio()
    dn, dk = d[0], d[1].bit_length() - 1
    assert d[1] == 1 << dk and 0 < dn < d[1]
    mant, expo = np.frexp(np.asarray(va, np.float32))
    assert np.all(mant == 0.5)
    j = (1 - expo).astype(np.int64)
    J = int(j.max())
    rp64, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    dangling = np.bincount(ci, minlength=n) == 0
    filled = np.flatnonzero(np.diff(rp64) > 0)
    R, e = np.ones(n, np.int64), k                                   # ranks = R * 2^-e
    for _ in range(steps):
        E = e + J + dk + k                                           # every quantity of the step is a multiple of 2^-E
        if E > 62:
            raise OverflowError("the step does not fit int64: not provable here")
        prod = R[ci] << (J - j)                                      # * 2^-(e + J)
        run = np.concatenate([[0], np.cumsum(prod)])
        acc = run[rp64[1:]] - run[rp64[:-1]]
        any_bit = np.bitwise_or.reduceat(prod, rp64[filled]) if filled.size else np.zeros(0, np.int64)
        quantum = any_bit & -any_bit                                 # per row: products are multiples of it ...
        exact = bool(np.all((acc[filled] >> 24) < quantum))          # ... and the row's sum is below 2^24 of them
        s = int(R[dangling].sum())                                   # * 2^-e: the dangling mass, float(double sum)
        dacc = dn * acc                                              # * 2^-(e + J + dk)
        ds = dn * s                                                  # d * s at 2^-(e + dk); d * s / n at 2^-(e + dk + k)
        tele = (1 << dk) - dn                                        # 1 - d at 2^-dk; (1 - d) / n at 2^-(dk + k)
        first = (dacc << k) + (ds << J)                              # d * acc + d * s / n
        fresh = first + (tele << (e + J))
        diff = fresh - (R << (E - e))
        exact = exact and all(_fits_float32(v) for v in (s, dacc, ds, tele, first, fresh, diff))
        exact = exact and int(fresh.sum()) == 1 << E                 # mass 1: the final r /= sum(r) divides by 1.0f
        square_sum = sum(int(v) * int(v) for v in diff[diff != 0])
        residual = math.ldexp(math.sqrt(square_sum), -E)
        low = int(np.bitwise_or.reduce(fresh))
        shift = (low & -low).bit_length() - 1
        R, e = fresh >> shift, E - shift
        yield np.ldexp(R.astype(np.float64), -e).astype(np.float32), residual, exact


def dyadic_pagerank(rp, ci, va, n, damping, steps):
    """(ranks float32, exact residual sqrt(sum (r_new - r_old)^2) of the last step as float64) after `steps` steps
    of r_new = d * (A r) + d * s / n + (1 - d) / n from r = 1 / n, s = the old ranks summed over the dangling nodes:
    the library's formula in integers."""
    assert steps >= 1
    for ranks, residual, _ in _dyadic_run(rp, ci, va, n, damping, steps):
        pass
    return ranks, residual


def dyadic_trajectory(rp, ci, va, n, damping, steps):
    """[(ranks float32, exact residual)] after step 1, 2, ... `steps`: what a test that looks after EVERY step wants."""
    return [(ranks, residual) for ranks, residual, _ in _dyadic_run(rp, ci, va, n, damping, steps)]


def exact_steps(rp, ci, va, n, damping, max_steps=4):
    """Number of leading steps (up to max_steps) in which everything the device computes is exact in float32: per
    row all products and the row's sum are multiples of one quantum q with sum < 2^24 q (check_exact's condition,
    scaled); s, d * acc, d * s, d * s / n, (1 - d), both partial sums of the update, r_new and r_new - r_old are
    representable; the ranks sum to exactly 1."""
    count = 0
    try:
        for _, _, exact in _dyadic_run(rp, ci, va, n, damping, max_steps):
            if not exact:
                break
            count += 1
    except OverflowError:
        pass
    return count


DYADIC_DAMPING = 0.5
DYADIC_DIRECT_N = 2048
DYADIC_DIRECT_DANGLING = (3, 64, 700, 701, 1024, 1500, 2046, 2047)         # a power-of-two count: d * s / n stays short
DYADIC_DIRECT = [("L%d" % L, L, (1, 2, 4) if L == 1 else (2 * L, 4 * L)) for L in LANES]
# name -> (n, W, R, dangling nodes, fold, pr_plan_after, steps wanted at least)
DYADIC_TILED = {
    "n16_4096x64_dangling_fold": (1 << 16, 4096, 64, 1 << 10, True, 0, 1),
    "n16_8192x1024_closed_fold": (1 << 16, 8192, 1024, 0, True, 0, 3),
    "n16_16384x9984_dangling_stream": (1 << 16, 16384, 9984, 1 << 10, False, 0, 1),
    "n18_4096x64_closed_stream": (1 << 18, 4096, 64, 0, False, 0, 3),
    "n18_8192x1024_dangling_fold": (1 << 18, 8192, 1024, 1 << 12, True, 0, 1),
    "n18_16384x9984_closed_fold": (1 << 18, 16384, 9984, 0, True, 0, 3),
    "n16_8192x1024_closed_switch_after_1": (1 << 16, 8192, 1024, 0, True, 1, 3),
    # dangling nodes drawn from the source-only nodes (DYADIC_SOURCES below): exact beyond step 1, so the dangling
    # mass the DEVICE accumulated in step k enters step k + 1 under a bit-exact comparison
    "n16_4096x64_sources_fold": (1 << 16, 4096, 64, 1 << 12, True, 0, 3),
    "n16_8192x1024_sources_stream": (1 << 16, 8192, 1024, 1 << 12, False, 0, 2),
    "n18_16384x9984_sources_fold": (1 << 18, 16384, 9984, 1 << 12, True, 0, 2),
    "n16_4096x64_sources_switch_after_1": (1 << 16, 4096, 64, 1 << 12, True, 1, 3),
}
# name -> hubs of the cases whose dangling nodes are source-only nodes.  Out-degrees (2, 4).  Shorter hubs keep the
# ranks short for one step more (three exact steps); the 5000 / 2500 pair is what the other tiled cases carry.
DYADIC_SOURCES = {
    "n16_4096x64_sources_fold": lambda n: [(n // 3, 700), (n - 1, 350)],
    "n16_8192x1024_sources_stream": lambda n: [(n // 3, 5000), (n - 1, 2500)],
    "n18_16384x9984_sources_fold": lambda n: [(n // 3, 5000), (n - 1, 2500)],
    "n16_4096x64_sources_switch_after_1": lambda n: [(n // 3, 700), (n - 1, 350)],
}
# the same construction for the direct kernel (n = 2^16 stays below the tiled engine's 2^20 entries): (name, L, degrees)
DYADIC_SOURCE_DIRECT = [("sources_L1", 1, (2, 4)), ("sources_L2", 2, (4, 8)), ("sources_L4", 4, (8, 16))]
SHARDED_CASE = "n16_4096x64_sources_fold"         # the graph tests/test_gpu_sharded_exact.py cuts (three exact steps)
_dyadic_cache = {}


def source_only_nodes(n, hubs):
    """The nodes dyadic_graph never links to: rows with row % 13 == 5 that are not hubs."""
    nodes = np.arange(5, n, 13, dtype=np.int64)
    return nodes[~np.isin(nodes, np.array([h for h, _ in hubs], np.int64))]


def source_only_dangling(rng, n, hubs, count):
    """`count` dangling nodes (a power of two) drawn from the source-only nodes.  Nobody links to them and they link
    to nobody, so after every step all of them carry the same short rank d * s / n + (1 - d) / n and their sum s stays
    short: the dangling term survives more than one exact step (a dangling node WITH in-links has a long rank after
    step 1).  Drawn four times as densely at the top of the node range as at its bottom, so that shards of equal
    rows own different numbers of them and a commit that reads one rank's partial mass for all shows."""
    assert count & (count - 1) == 0
    nodes = source_only_nodes(n, hubs)
    weight = 1.0 + 3.0 * np.arange(nodes.size) / nodes.size
    return np.sort(rng.choice(nodes, size=count, replace=False, p=weight / weight.sum()))


def dyadic_case(name):
    """(n, row_ptrs, cols, vals, steps, ranks, residual) of a direct ("L8") or tiled (DYADIC_TILED) case: steps =
    exact_steps, ranks / residual = dyadic_pagerank at that count (None when steps == 0)."""
    if name in _dyadic_cache:
        return _dyadic_cache[name]
    if name in DYADIC_SOURCES:
        n, _, _, dangling_count, _, _, _ = DYADIC_TILED[name]
        rng = np.random.default_rng(sum(name.split("x")[0].encode()))       # cases that differ in W, R only share a graph
        hubs = DYADIC_SOURCES[name](n)
        dangling = source_only_dangling(rng, n, hubs, dangling_count)
        degrees = (2, 4)
    elif name.startswith("sources_L"):
        index, (_, L, degrees) = next((i, c) for i, c in enumerate(DYADIC_SOURCE_DIRECT) if c[0] == name)
        n = 1 << 16
        rng = np.random.default_rng(300 + index)
        hubs = [(n // 3, 700), (n - 1, 350)]
        dangling = source_only_dangling(rng, n, hubs, 1 << 12)
    elif name in DYADIC_TILED:
        n, _, _, dangling_count, _, _, _ = DYADIC_TILED[name]
        rng = np.random.default_rng(sum(name.encode()))
        dangling = rng.choice(n, size=dangling_count, replace=False)
        degrees = (2, 4, 8, 16) if dangling_count else (1, 2)
        hubs = [(n // 3, 5000), (n - 1, 2600)]                             # beyond the long-row limit 8 * strips (<= 512 here)
        if dangling_count:
            hubs.append((n // 3 + 1, 700))                                 # (link 2 of a column: out-degree > 2 only)
    else:
        index, (_, L, degrees) = next((i, c) for i, c in enumerate(DYADIC_DIRECT) if c[0] == name)
        n, dangling = DYADIC_DIRECT_N, np.array(DYADIC_DIRECT_DANGLING)
        rng = np.random.default_rng(600 + index)
        hubs = [(n // 3, 1500), (n - 1, 600)]
    rp, ci, va = dyadic_graph(rng, n, degrees, dangling, hubs)
    steps = exact_steps(rp, ci, va, n, DYADIC_DAMPING)
    ranks, residual = dyadic_pagerank(rp, ci, va, n, DYADIC_DAMPING, steps) if steps else (None, None)
    _dyadic_cache[name] = (n, rp, ci, va, steps, ranks, residual)
    return _dyadic_cache[name]


def tiled_debug(W, R, extra=""):
    """The SPMV_DEBUG string that pushes a small matrix through the tiled engine at strip width W, tile height R."""
    return "min_cols=1,min_nnz=1,strip=%d,tile=%d%s" % (W, R, "," + extra if extra else "")


# ------------------------------------------------------------------------------------------ sharded PageRank catalogue
# How tests/test_gpu_sharded_exact.py cuts SHARDED_CASE.  tests/test_exact_data.py proves on the CPU what each cut
# claims (an empty shard, a hub alone, a block boundary inside a strip ...) and that the dangling nodes are spread
# over the ranks with different masses.
SHARD_WORLDS = (1, 2, 3, 5, 8)
SHARD_W, SHARD_R = 4096, 64                  # strip width / tile height where the shards run the tiled engine
SHARD_ALIGNS = (4096, 8192, 1000)            # = W, a multiple of W, smaller than W and not dividing it
SHARD_CHUNKS = (2, 3, 4, 7)


def equal_row_bounds(n, world):
    """Layout's default cut (pagerank_dist.py): ceil(n / world) rows per rank, rounded up to even when world > 1."""
    shard_len = -(-n // world)
    if world > 1 and shard_len % 2:
        shard_len += 1
    return np.minimum(np.arange(world + 1, dtype=np.int64) * shard_len, n)


def shard_cut_edges(n, hub):
    """name -> explicit bounds; `hub` is a hub row (n - 1 is the other one).  Row 5 is a source-only, empty row."""
    return {
        "empty_first": [0, 0, 30001, n], "empty_middle": [0, 30001, 30001, n], "empty_last": [0, 30001, n, n],
        "one_empty_row": [0, 5, 6, n],                       # rows but no entries
        "hub_alone": [0, hub, hub + 1, n], "last_hub_alone": [0, 30000, n - 1, n],
        "cut_before_hub": [0, hub, n], "cut_after_hub": [0, hub + 1, n],
        "odd_lengths": [0, 25539, 45540, n],                 # the longest shard is odd: rounded up to even
    }


def chunk_world(n, chunks):
    """(world, bounds) of a chunk-major case: two equal shards for even chunk counts, else three shards of 30 000,
    22 000 and the remaining rows (short shards: their last pieces hold no rows)."""
    return (2, None) if chunks % 2 == 0 else (3, [0, 30000, 52000, n])


def dangling_per_rank(bounds, dangling):
    """Number of dangling nodes each rank owns (their ranks are all equal, so the masses are in this proportion)."""
    bounds = np.asarray(bounds, np.int64)
    return np.bincount(np.searchsorted(bounds[1:-1], np.asarray(dangling), side="right"), minlength=bounds.size - 1)


# ------------------------------------------------------------------------------------------ plan-geometry catalogue
# Every case: a small matrix and the SPMV_DEBUG string under which the tiled engine must build the plan the case
# claims (strip width W, tile height R, strips, tiles, long rows or none, folded values or a value stream, and where
# the construction fixes them the slot, item and long-row counts).  tests/test_exact_data.py proves the data exact
# and W / R from the host logic; tests/test_gpu_tiled_geometry.py asserts the rest from csr_tiled_info.
def default_long_row(strips):
    """build_plan (csrc/tiled_build.hip): rows with more entries than max(64, min(4096, 8 * strips)) are long."""
    return max(64, min(4096, 8 * strips))


def _scattered(rng, rows, cols, W, max_len=40):
    """Ragged rows of up to max_len random columns, every 11th row empty, plus entries at local columns 0 and W - 1
    of every strip, in the matrix's last column (the last, partial strip) and in its last row."""
    lens = rng.integers(0, max_len + 1, size=rows)
    lens[::11] = 0
    rr = np.repeat(np.arange(rows), lens)
    cc = rng.integers(0, cols, size=rr.size)
    edges = sorted({c for s in range(-(-cols // W)) for c in (s * W, min(s * W + W - 1, cols - 1))} | {cols - 1})
    er = np.concatenate([rng.integers(0, rows, size=3 * len(edges)), np.full(len(edges), rows - 1)])
    ec = np.concatenate([np.repeat(edges, 3), edges])
    return np.concatenate([rr, er]), np.concatenate([cc, ec])


def _row_deltas(rng, R):
    """Two tiles of R = 9984 rows, four strips of 4096 columns.  Strip 0: rows 1, 254, 255, 256, 509, 510, 511 apart
    in one cell; strip 1: rows 0 and R - 1 (9983 apart: 39 skip markers); strip 2: its only entry in the tile's last
    row (tile 0), an empty cell (tile 1); strip 3: a scattered background.  Tile 1 repeats it seven rows down."""
    rr, cc = [], []
    steps = np.cumsum([0, 1, 254, 255, 256, 509, 510, 511])
    for tile, shift in ((0, 0), (1, 7)):
        base = tile * R
        for r in steps + shift:
            for c in rng.choice(4096, size=int(rng.integers(1, 4)), replace=False):
                rr.append(base + r), cc.append(c)
        rr += [base + shift, base + shift, base + R - 1]
        cc += [4096 + 5, 4096 + 4095, 4096 + 17]
        if tile == 0:
            rr.append(base + R - 1), cc.append(2 * 4096)
    back_r = rng.integers(0, 2 * R, size=6000)
    return np.concatenate([rr, back_r]), np.concatenate([cc, 3 * 4096 + rng.integers(0, 4096, size=6000)])


ITEM_STRIP_ENTRIES = (1023, 1024, 1025, 4096, 0, 2048)     # per strip; the last one half in tile 0, half in tile 1
ITEM_SLOTS = 1024 + 1024 + 1028 + 4096 + 0 + 2048          # cells are padded to multiples of four slots
ITEMS_AT_1024 = 1 + 1 + 2 + 4 + 0 + 2                      # ceil(slots / 1024) per strip
ITEMS_AT_DEFAULT = 5                                       # default item size max(4096, W): one per non-empty strip


def _item_strips(rng):
    """Two tiles of 1024 rows, six strips of 4096 columns holding ITEM_STRIP_ENTRIES entries in consecutive rows (no
    skip markers), so that every strip's slot count is known: an item that ends at a cell end (strip 5 at item=1024),
    a strip of several items, strips of exactly one, a strip shorter than one item and an empty strip."""
    rr, cc = [], []
    for strip, count in enumerate(ITEM_STRIP_ENTRIES):
        i = np.arange(count)
        rows = i % 1024 if strip < 5 else i            # strip 5: rows 0..2047, one entry each
        rr.append(rows), cc.append(strip * 4096 + (i // 1024) * 7 + (rows * 13) % 5 + 100 * (i // 1024))
    return np.concatenate(rr), np.concatenate(cc)


LONG_LIMIT = 64                                            # long_cap=64,long_factor=1
LONG_ROW_LENGTHS = {10: 64, 20: 65,                        # tile 0: exactly the limit (short), one more (long)
                    70: 512, 80: 513, 100: 1024,           # tile 1: three long rows; 512-entry chunks: 1, 2, 2
                    130: 65, 140: 100, 150: 200, 160: 66, 191: 90,      # tile 2: long rows only
                    255: 5000}                             # tile 3: the matrix's last row


def _long_rows(rng):
    """Four tiles of 64 rows, three strips: LONG_ROW_LENGTHS, short ragged rows elsewhere except in tile 2."""
    rows, cols = 256, 3 * 4096
    lens = rng.integers(0, 20, size=rows)
    lens[128:192] = 0
    for r, n in LONG_ROW_LENGTHS.items():
        lens[r] = n
    rr = np.repeat(np.arange(rows), lens)
    return rr, np.concatenate([rng.choice(cols, size=n, replace=False) for n in lens])      # distinct: lengths hold


def _geometry_cases():
    cases = {}

    def add(name, rows, cols, W, R, structure, fold, extra="", **expect):
        strips, tiles = -(-cols // W), -(-rows // R)
        cases[name] = dict(name=name, rows=rows, cols=cols, W=W, R=R, strips=strips, tiles=tiles, fold=fold,
                           debug=tiled_debug(W, R, extra), structure=structure, long_rows=0, **expect)

    for W in (4096, 8192, 16384, 32768):                   # strip width x fold x columns around a strip end
        s = 2 if W == 32768 else 3
        for fold in (False, True):
            for off in (-1, 0, 1):
                cols = s * W + off
                add("strip_%d_%s_cols%+d" % (W, "fold" if fold else "stream", off), 3000, cols, W, 1024,
                    lambda rng, cols=cols, W=W: _scattered(rng, 3000, cols, W), fold)
    for R, t in ((64, 3), (128, 3), (1024, 3), (4800, 2), (9984, 2)):      # tile height x rows around a tile end
        for off in (-1, 0, 1):
            rows = t * R + off
            add("tile_%d_rows%+d" % (R, off), rows, 10000, 4096, R,
                lambda rng, rows=rows: _scattered(rng, rows, 10000, 4096), fold=(off == 0))
    for fold in (False, True):
        tag = "fold" if fold else "stream"
        add("row_deltas_" + tag, 2 * 9984, 4 * 4096, 4096, 9984, lambda rng: _row_deltas(rng, 9984), fold)
        add("items_1024_" + tag, 2048, 6 * 4096, 4096, 1024, _item_strips, fold, extra="item=1024",
            items=ITEMS_AT_1024, slots=ITEM_SLOTS)
        add("items_default_" + tag, 2048, 6 * 4096, 4096, 1024, _item_strips, fold,
            items=ITEMS_AT_DEFAULT, slots=ITEM_SLOTS)
        add("long_rows_" + tag, 256, 3 * 4096, 4096, 64, _long_rows, fold, extra="long_cap=64,long_factor=1")
        cases["long_rows_" + tag]["long_rows"] = sum(n > LONG_LIMIT for n in LONG_ROW_LENGTHS.values())
    return cases


GEOMETRY_CASES = _geometry_cases()
GEOMETRY_NAMES = list(GEOMETRY_CASES)
BUILDER_FORM_NAMES = ["strip_8192_stream_cols+1", "row_deltas_stream", "long_rows_fold"]
ENTRY_POINT_GEOMETRIES = [(4096, 64), (16384, 9984)]
_geometry_cache = {}


def geometry_matrix(name):
    """(case, row_ptrs, cols, vals, x): distinct (row, column) pairs in row-major order; values one integer weight
    per column when the case folds, else drawn per entry; checked exact."""
    if name not in _geometry_cache:
        case = GEOMETRY_CASES[name]
        rng = np.random.default_rng(sum(name.encode()))
        rr, cc = case["structure"](rng)
        keys = np.unique(np.asarray(rr, np.int64) * case["cols"] + np.asarray(cc, np.int64))
        rr, ci = keys // case["cols"], (keys % case["cols"]).astype(np.int32)
        rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=case["rows"]))]).astype(np.int32)
        if case["fold"]:
            weight = (rng.integers(1, 9, size=case["cols"]) * rng.choice([-1, 1], size=case["cols"])).astype(np.float32)
            va = weight[ci]
        else:
            va = (rng.integers(1, 9, size=ci.size) * rng.choice([-1, 1], size=ci.size)).astype(np.float32)
        x = rng.integers(-64, 65, size=case["cols"]).astype(np.float32)
        check_exact(rp, ci, va, x)
        _geometry_cache[name] = (case, rp, ci, va, x)
    return _geometry_cache[name]


def entry_matrix(W, R):
    """3 * R + 1 rows (a last tile of one row) x 2 * W + 1 columns (a last strip of one column), rows of up to 8
    scattered entries plus the strip-edge entries (the last row holds one per strip edge on top): a width the ELL
    slabs can carry."""
    rows, cols = 3 * R + 1, 2 * W + 1
    rng = np.random.default_rng(W + R)
    rr, cc = _scattered(rng, rows, cols, W, max_len=8)
    keys = np.unique(rr.astype(np.int64) * cols + cc)
    rr, ci = keys // cols, (keys % cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=rows))]).astype(np.int32)
    va = (rng.integers(1, 9, size=ci.size) * rng.choice([-1, 1], size=ci.size)).astype(np.float32)
    return rows, cols, rp, ci, va


def entry_point_systems(W):
    """The integer SPD and non-symmetric systems the solvers' tiled route runs at strip width W: n = 20 011, so that
    4096-column strips give five of them and 9984-row tiles three."""
    n = 20011
    return integer_spd(n, 50000, seed=W), integer_nonsym(n, 90000, seed=W + 1)


BICG_ALPHA_INVERSE = 64


def bicgstab_first_step_system(n, offdiagonal, seed, K=BICG_ALPHA_INVERSE):
    """(n, row_ptrs, cols, vals, b) of a non-symmetric, strictly row diagonally dominant integer system S + D built so
    that BiCGSTAB's first step from x0 = 0 without a preconditioner stays exact: b holds non-zero integers in
    [-64, 64] and the diagonal is K + delta_i, |delta_i| <= 8, with sum_i delta_i b_i^2 == -b.(S b), so that
    b.(A b) == K b.b and alpha = rho / (rhat.v) == 1 / K exactly (K a power of two).  Then s = b - (A b) / K is a
    vector of multiples of 1 / K and t = A s is exact as well (bicgstab_first_step)."""
    rng = np.random.default_rng(seed)
    r, c, v = _integer_offdiagonal(rng, n, offdiagonal, 3)
    b = rng.integers(1, 65, size=n) * rng.choice([-1, 1], size=n)
    sb = np.bincount(r, weights=v * b[c], minlength=n).astype(np.int64)
    target = -int(b @ sb)
    delta = np.zeros(n, np.int64)
    for m in range(64, 0, -1):                       # coin change over b_i^2, largest first; |b| == 1 takes the rest
        rows = np.flatnonzero(np.abs(b) == m)
        if rows.size == 0:
            continue
        q = max(-8 * rows.size, min(8 * rows.size, int(target / (m * m))))       # rounded towards zero
        base, extra = divmod(abs(q), rows.size)
        delta[rows] = np.sign(q) * base
        delta[rows[:extra]] += np.sign(q)
        target -= q * m * m
    assert target == 0 and np.abs(delta).max() <= 8
    d = K + delta
    assert np.all(d > np.bincount(r, weights=np.abs(v), minlength=n))            # strictly dominant
    diag = np.arange(n)
    n, rp, ci, va = _csr_from_triplets(n, np.concatenate([r, diag]), np.concatenate([c, diag]), np.concatenate([v, d]))
    return n, rp, ci, va, b.astype(np.float32)


def bicgstab_first_step(rp, ci, va, b, K=BICG_ALPHA_INVERSE):
    """x after ONE BiCGSTAB step from x0 = 0, no preconditioner, under bicgstab.h's rules, for a system of
    bicgstab_first_step_system: p = rhat = r = b, v = A b (integers), alpha = fp32(b.b / b.v) = 1 / K, s = r - alpha v
    (multiples of 1 / K, exact), t = A s (exact), omega = fp32(t.s / t.t) (integer dot products scaled by K^-2, below
    2^53: exact in fp64 in any order, one division, one rounding), x = fma(omega, s, fma(alpha, p, 0)): alpha p is
    exact and omega s + alpha p has fewer than 53 significant bits, so fp64 holds it exactly and the fp32 rounding of
    that is the fused result.  Every claim is asserted here.  Returns (x float32, omega)."""
    b64 = np.asarray(b).astype(np.int64)
    check_exact(rp, ci, va, b)
    v = exact_reference(rp, ci, va, b).astype(np.int64)
    assert int(b64 @ v) == K * int(b64 @ b64)                                    # alpha == 1 / K
    ks = K * b64 - v                                                             # K s
    ks32 = ks.astype(np.float32)
    check_exact(rp, ci, va, ks32)
    kt = exact_reference(rp, ci, va, ks32).astype(np.int64)                      # K t
    ts, tt = int(kt @ ks), int(kt @ kt)
    assert 0 < tt < 2**53 and abs(ts) < 2**53 and ts != 0
    omega = np.float32(np.float64(ts) / np.float64(tt))
    mant, expo = np.frexp(np.float64(omega))
    w_int, w_exp = int(mant * 2**24), int(expo) - 24                             # omega == w_int * 2^w_exp
    assert np.float64(w_int) * 2.0**w_exp == np.float64(omega) and w_exp <= 0
    scaled = w_int * ks.astype(object) + (b64.astype(object) << -w_exp)          # K 2^-w_exp (omega s + b / K)
    assert max(abs(int(u)) for u in scaled) < 2**53
    x = (np.float64(omega) * (ks.astype(np.float64) / K) + b64.astype(np.float64) / K).astype(np.float32)
    return x, omega


# ------------------------------------------------------------------------------------------ array-view catalogue
# The matrices tests/test_gpu_array_views.py hands to the library as VIEWS into larger device allocations: every array
# starts 0..3 elements past a 16-byte boundary and is surrounded by poison that is legal to read (it can never fault)
# but cannot pass unnoticed in a result.  x is drawn from NON-ZERO integers and no stored value is zero, so one stray
# entry of any kind (a neighbour's live entry, the poison column num_cols - 1, the poison value 2^22, the x poison 2^22)
# moves a row's sum by a non-zero integer; tests/test_exact_data.py proves that for every member.
VIEW_NAMES = ["sweep:L1_low", "sweep:L4_top", "sweep:L16_low", "sweep:L64_top", "ldsx:L4_top",
              "merge:row_end_T-1",                       # tile 0's last merge item is a row end
              "merge:row_over_four_tiles",               # tiles 1 and 2 lie inside one long row
              "tiled:4096x64"]                           # ENTRY_POINT_GEOMETRIES[0]: the tiled engine's smallest plan
VIEW_OFFSETS = [(0, 0, 0), (1, 1, 1), (2, 3, 1), (3, 1, 2), (1, 2, 3)]      # (row_ptrs, cols, vals) elements past 16 bytes
VIEW_POISON = float(1 << 22)                             # value and x poison


def nonzero_x(rng, count, xmax=64):
    """Non-zero integers in [-xmax, xmax] as float32."""
    return (rng.integers(1, xmax + 1, size=count) * rng.choice([-1, 1], size=count)).astype(np.float32)


def view_matrix(name):
    """dict(kind, L, rows, num_cols, rp, ci, va, x) of one VIEW_NAMES member: the catalogue's matrix under a non-zero
    x; L is what the lane rule gives it; "tiled" members carry W and R."""
    kind, key = name.split(":")
    extra = {}
    if kind == "sweep":
        _, rp, ci, va, _ = sweep_matrix(key)
        num_cols = SWEEP_COLS
    elif kind == "ldsx":
        _, num_cols, rp, ci, va, _ = ldsx_matrix(key)
    elif kind == "merge":
        rp, ci, va, _ = merge_cut_matrix(key)
        num_cols = MERGE_CUT_COLS
    else:
        W, R = (int(v) for v in key.split("x"))
        _, num_cols, rp, ci, va = entry_matrix(W, R)
        extra = dict(W=W, R=R)
    rows = len(rp) - 1
    x = nonzero_x(np.random.default_rng(sum(name.encode())), num_cols)
    check_exact(rp, ci, va, x)
    return dict(kind=kind, key=key, L=lanes_for(int(rp[-1]), rows), rows=rows, num_cols=num_cols, rp=rp, ci=ci, va=va,
                x=x, **extra)


# ------------------------------------------------------------------------------------------ one-hot Krylov systems
# GMRES (csrc/gmres.hip) held to the bit along the whole basis walk.  A = D + B, D diagonal, B one entry per column i
# at row (i + s) mod n, every stored value +- a power of two, b = 2^a e_p.  Then A e_i = d_i e_i + beta_i e_(i+s): from
# x0 = 0 the Arnoldi vectors of the FIRST cycle are v_j = +- e_(q_j), q_j = (p + j s) mod n, as long as the walk does
# not come back to a position: h1 holds d_(q_j) at i = j and exact zeros elsewhere, h2 is exactly zero, h_j+1 =
# |beta_(q_j)|, every dot product has at most one non-zero term.  The small problem (rotations, back-substitution) is a
# fixed sequence of rounded fp64 operations, the same on the host and on the device.  At a close, A x touches at most
# two non-zero products per row, both exact (powers of two), so one rounded addition whatever the order.
#
# From the SECOND cycle on the vectors are no longer one-hot: r = b - A x is supported on q_0..q_k, and every later
# vector on the positions walked so far (after `it` steps: q_0..q_it).  Dot products then sum up to it + 1 exact fp64
# products and their last fp64 bits depend on the order; what the solver takes from them is rounded to fp32 (h1, h2,
# 1 / beta, 1 / h_j+1, y), which hides that unless a value sits within a few fp64 ulps of an fp32 rounding boundary.
# tests/test_exact_data.py probes this per case with three summation orders (numpy's, its reverse, the correctly
# rounded sum) and demands the same bits from all of them.  |d| is 1 or 2 and |beta| 1/2, 1 or 2: the solution neither
# decays nor grows along the walk by more than a few powers of ten in 129 steps, so nothing comes near fp32's
# subnormal range, and the small problem stays well enough conditioned that an order change is not amplified.
ONEHOT_CHUNK = 1024                  # kChunk (csrc/gmres.hip): elements of w a workgroup of a basis kernel holds
ONEHOT_ORTHO_BLOCKS = 256            # kOrthoBlocks: beyond 256 chunks the basis kernels take a second grid-stride trip
ONEHOT_FOLD_LANES = 64               # fold_columns: beyond 64 workgroups a lane folds a second partial
ONEHOT_ROW_BLOCKS = 2048             # kMaxResidentBlocks: gmres_spmv<L> / gmres_residual<L> run at most that many
ONEHOT_RHS = 4.0                     # b = 2^2 e_p


def gmres_onehot_system(n, p, s, steps, seed, empty_column=None):
    """dict(n, rp, ci, va, b, walk, d, beta): the one-hot system above.  `walk` holds q_0..q_steps, the positions
    anything can reach within `steps` Arnoldi steps; asserted distinct, and nothing off the walk feeds into it.  Each
    row stores its diagonal entry and the entry of column (row - s) mod n, in an order drawn per row.
    empty_column = j: B's column q_j stays empty, so A e_(q_j) = d e_(q_j) and step j finds h_j+1 == 0."""
    assert 0 <= p < n and 0 < s < n and steps + 1 <= n
    rng = np.random.default_rng(seed)
    walk = (p + s * np.arange(steps + 1, dtype=np.int64)) % n
    assert np.unique(walk).size == steps + 1, "the walk revisits a position"
    assert (p - s) % n not in set(walk.tolist())
    d = np.ldexp(rng.choice([-1.0, 1.0], size=n), rng.integers(0, 2, size=n)).astype(np.float32)
    beta = np.ldexp(rng.choice([-1.0, 1.0], size=n), rng.integers(-1, 2, size=n)).astype(np.float32)
    idx = np.arange(n, dtype=np.int64)
    rows = np.concatenate([idx, (idx + s) % n])
    cols = np.concatenate([idx, idx])
    vals = np.concatenate([d, beta])
    keep = np.ones(2 * n, bool)
    if empty_column is not None:
        keep[n + int(walk[empty_column])] = False
    first = rng.integers(0, 2, size=n)                         # 1: the off-diagonal entry is stored first
    key = 2 * rows + (np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64)]) ^ first[rows])
    order = np.argsort(key[keep], kind="stable")
    rows, cols, vals = rows[keep][order], cols[keep][order], vals[keep][order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    b = np.zeros(n, np.float32)
    b[p] = ONEHOT_RHS
    return dict(n=n, rp=rp, ci=cols.astype(np.int32), va=vals.astype(np.float32), b=b, walk=walk, d=d, beta=beta,
                empty_column=empty_column)


def onehot_compact(system):
    """(m, rp, ci, va, b) of the system restricted to its walk, in walk order: row j is row q_j with its entries in
    storage order, those whose column lies off the walk dropped (x is 0 there from start to end)."""
    walk = system["walk"]
    at = {int(q): j for j, q in enumerate(walk)}
    rp, ci, va = system["rp"], system["ci"], system["va"]
    c_rp, c_ci, c_va = [0], [], []
    for q in walk:
        for e in range(int(rp[q]), int(rp[q + 1])):
            if int(ci[e]) in at:
                c_ci.append(at[int(ci[e])])
                c_va.append(va[e])
        c_rp.append(len(c_ci))
    return (walk.size, np.array(c_rp, np.int32), np.array(c_ci, np.int32), np.array(c_va, np.float32),
            system["b"][walk].copy())


def gmres_onehot_reference(system, restart, max_iterations, precond):
    """gmres_cases.restate on the walk positions only, scattered back: (x, iterations, restarts, converged, breakdown,
    relative residual) for tolerance 0 from x0 = 0.  tests/test_exact_data.py shows that it equals restate on the
    whole system in every field at small n."""
    import gmres_cases as gc
    m, rp, ci, va, b = onehot_compact(system)
    out = gc.restate(m, rp, ci, va, b, np.zeros(m, np.float32), 0.0, max_iterations, restart, precond)
    x = np.zeros(system["n"], np.float32)
    x[system["walk"]] = out[0]
    return (x,) + tuple(out[1:])


def _onehot_cases():
    cases = {}

    def add(name, n, p, s, restart, visits=(), chunks=(), empty_column=None, max_iterations=None):
        it = 2 * restart + 1 if max_iterations is None else max_iterations
        cases[name] = dict(name=name, n=n, p=p, s=s, restart=restart, max_iterations=it, visits=tuple(visits),
                           chunks=tuple(chunks), empty_column=empty_column, seed=len(cases) + 17)

    # groups of eight: two full cycles and one column more, n = 4103 (3 mod 4; 4 * 1026 = n + 1, so every fourth step
    # moves one element on: n-3, 1023, 2049, 3075, n-2, 1024, ...)
    for m in (1, 2, 7, 8, 9, 30, 64):
        add("restart_%d" % m, 4103, 4100, 1026, m, visits=(4100, 1023) if m < 7 else (4100, 4101, 4102, 0, 1023, 1024))
    # vector tails at n mod 4 = 1 and 2 (3 * 1026 = 3077 + 1, 3 * 1025 = 3074 + 1)
    add("tail_n3077", 3077, 3074, 1026, 9, visits=(3074, 3075, 3076, 0, 1023, 1024))
    add("tail_n3074", 3074, 3071, 1025, 9, visits=(3071, 3072, 3073, 0, 1023, 1024))
    # 129 workgroups: fold_columns' lanes 0 fold partials 0, 64 and 128
    add("fold_second_trip", 131587, 5, 65540, 9, visits=(5, 65545, 131085), chunks=(0, 64, 128))
    # 259 chunks on 256 workgroups: the chunks below, at and past 256 (element 262 144), and the last, partial f32x4
    add("grid_second_trip", 264195, 260102, 1023, 9, visits=(261125, 262148, 263171, 264194), chunks=(254, 255, 256, 257, 258, 0))
    # L = 1: 2048 workgroups of 256 rows; rows 524 291 and 525 314 belong to the second trip of the row loops
    add("rows_second_trip", 525315, 523268, 1023, 9, visits=(523268, 524291, 525314, 1022))
    # B's column q_5 empty: six exact columns, then h_6 == 0 closes the cycle three steps before the host expects it
    add("early_close", 4103, 4100, 1026, 9, visits=(4100, 1023, 4101), empty_column=5)
    return cases


ONEHOT_CASES = _onehot_cases()
ONEHOT_NAMES = list(ONEHOT_CASES)
_onehot_cache = {}


def onehot_case(name):
    """(case, system) of one ONEHOT_CASES member; the system is built once."""
    if name not in _onehot_cache:
        c = ONEHOT_CASES[name]
        _onehot_cache[name] = (c, gmres_onehot_system(c["n"], c["p"], c["s"], c["max_iterations"], c["seed"],
                                                      c["empty_column"]))
    return _onehot_cache[name]


# ------------------------------------------------------------------------------------------ GMRES, first step
def pm_one_rhs(n, k, seed):
    """+-1 on exactly 4^k positions, 0 elsewhere: ||b|| = 2^k."""
    assert 4 ** k <= n
    rng = np.random.default_rng(seed)
    b = np.zeros(n, np.float32)
    b[rng.choice(n, size=4 ** k, replace=False)] = rng.choice([-1.0, 1.0], size=4 ** k)
    return b


def gmres_first_step(rp, ci, va, b, k):
    """x after ONE GMRES step from x0 = 0 without a preconditioner under gmres.h's rules, for an integer matrix and a
    +-1 / 0 right-hand side with 4^k non-zeros (pm_one_rhs).  beta = 2^k and v_0 = b / 2^k exactly; w = A b / 2^k holds
    integers over 2^k; h1_0 = b.A b / 4^k is an exact fp32 value; fmaf(-h1_0, v_0, w) = (4^k (A b)_i - b_i (b.A b)) / 8^k
    with a numerator below 2^24: exact; h2_0 = (b.A b - (b.A b)(b.b) / 4^k) / 4^k == 0; w.w is a sum of integers over
    64^k that stays below 2^53: exact in fp64 in any order.  What follows is the one-column small problem in fp64 (one
    square root, rounded products and sums, two divisions) and x1 = fp32(y_0) v_0, an exact product.  Every claim is
    asserted.  Returns (x1 float32, y_0 float64)."""
    b = np.asarray(b, np.float32)
    check_exact(rp, ci, va, b)
    b64 = b.astype(np.int64)
    scale = 4 ** k
    assert set(np.unique(b64).tolist()) <= {-1, 0, 1} and int(np.abs(b64).sum()) == scale == int(b64 @ b64)
    ab = exact_reference(rp, ci, va, b).astype(np.int64)                         # 2^k w
    bab = int(b64 @ ab)
    h1 = np.float32(np.float64(bab) / np.float64(scale))
    assert np.float64(h1) * scale == bab and abs(bab) < EXACT_LIMIT             # an exact fp32 value
    num = scale * ab - b64 * bab                                                 # 8^k (w after the first update)
    assert int(np.abs(num).max()) < EXACT_LIMIT                                  # ... which fp32 holds: the fmaf is exact
    assert int(b64 @ num) == 0                                                   # h2_0 == 0: the second update changes nothing
    ww_int = sum(int(v) * int(v) for v in num[num != 0])                         # 64^k w.w
    assert 0 < ww_int < 2 ** 53
    one = np.float64(1.0)
    ww = np.float64(ww_int) / np.float64(64 ** k)
    beta = np.float64(2 ** k)
    hn = np.sqrt(ww)
    a = np.float64(h1) + np.float64(np.float32(0.0))
    d = np.sqrt(a * a + hn * hn)
    assert np.isfinite(d) and d > 0 and hn > 0
    c = a / d
    g0 = c * beta
    y0 = g0 / d
    x1 = (np.float64(np.float32(y0)) * (b.astype(np.float64) / beta)).astype(np.float32)
    assert np.array_equal(x1.astype(np.float64) * beta, np.float64(np.float32(y0)) * b.astype(np.float64) * one)
    return x1, y0


GMRES_STEP_K = 5                              # 1024 of the 1201 / 1202 rows of solver_system
GMRES_TILED_STEP_K = 7                        # 16 384 of the 20 011 rows of entry_point_systems


def gmres_step_system(name):
    """(L, n, rp, ci, va, b) of solver_system(name, symmetric=False) with the +-1 / 0 right-hand side."""
    L, n, rp, ci, va, _, _ = solver_system(name, symmetric=False)
    return L, n, rp, ci, va, pm_one_rhs(n, GMRES_STEP_K, 1300 + SOLVER_NAMES.index(name))


def gmres_tiled_step_system(W):
    """(n, rp, ci, va, b): the non-symmetric system of entry_point_systems(W) with the +-1 / 0 right-hand side."""
    n, rp, ci, va = entry_point_systems(W)[1]
    return n, rp, ci, va, pm_one_rhs(n, GMRES_TILED_STEP_K, 1400 + W)


# ------------------------------------------------------------------------------------------ two-eigenvalue systems
# cg_solve / bicgstab_solve held to the bit to their LAST step, past the grid caps of csrc/solver_common.h
# (tests/test_gpu_solver_trips.py).  The rows fall into two sets S1 and S2, dealt by a fixed pseudo-random permutation;
# off-diagonal entries are integers and connect rows of one set only; every diagonal entry is d = 2^14; the
# off-diagonal row sums are prescribed, so the vector that is constant on a set and zero elsewhere is an eigenvector.
# b is constant on each set: a sum of two eigenvectors, and both Krylov methods end after two steps with r == 0.
#   CG        symmetric, row sums d/4 on S1 and d on S2, |b1|^2 == 2 |b2|^2:
#             alpha = 2/d, 2/d and beta = 1/2 (NONE); alpha = 2, 2 and beta = 1/2 (JACOBI, z = r / d)
#   BiCGSTAB  non-symmetric, row sums d/4 on S1 and -d/4 on S2, |b1|^2 == 3 |b2|^2:
#             alpha = 8/d, omega = -2/d, beta = 3, alpha = -2/d (NONE; times d with JACOBI), s == 0 at the half step
# A set's rows are cut into groups of g rows; inside a group, row q holds c_k at the rows q + k (and q - k when
# symmetric) mod g for k = 1..t, with t and g drawn per group (ragged rows) and sum_k c_k the prescribed value.  A +-1
# similarity A' = S A S, b' = S b varies the signs.  The scaled variant A' = T A T, b' = T b, T a power of two per row,
# has the diagonal d T^2: JACOBI's dinv then differs from row to row, and diag(sqrt(d) T) is an exact IC factor, diag(d T^2)
# an exact U (L = I).  CG's r.z and p.q do not see T; BiCGSTAB's dot products do, so there T is 2 on exactly three
# times as many rows of S1 as of S2, and the weights T^2 b^2 keep the ratio 3.
# n is padded with diagonal-only rows: for CG up to two rows of S2 with b = +-3 (n = 3 n2 + 19 f, f = n mod 3), for
# BiCGSTAB up to three rows with b = 0 (a diagonal-only row has the eigenvalue 1 under JACOBI, which no set shares).
# tests/test_exact_data.py runs cg.h's and bicgstab.h's algorithms in integers on every system and asserts each claim.
VEC_TRIP = 1024 * 256                        # kVecBlocks * kBlock: elements per trip of the element-wise kernels
ROW_TRIP_THREADS = 2048 * 256                # kMaxResidentBlocks * kBlock: a row kernel's trip is this / L rows
TWO_EIG_D = 1 << 14                          # the common diagonal; lambda = d / 4


def row_trip(L):
    return ROW_TRIP_THREADS // L


TRIP_SIZES = [257, 1201, VEC_TRIP, VEC_TRIP + 1, VEC_TRIP + 257, 2 * VEC_TRIP + 3, row_trip(1) + 257]
LANE_SIZES = {L: row_trip(L) + 256 // L + 1 for L in LANES[1:]}
TILED_TRIP_SIZE = VEC_TRIP + 257


def _circulant_rows(rng, members, t_choices, target, symmetric):
    """(rows, cols, vals) of one set's off-diagonal entries: `members` cut into groups, each with its own t (entries
    per direction) and g >= 2 t + 1 (t + 1 when not symmetric) rows, so that a row's columns are distinct; the weights
    c_1..c_t of a group are non-zero integers, +-1..3 but for the last, which brings their sum to `target` (half of it
    per direction when symmetric).  t == 0: rows without off-diagonal entries (target 0 only)."""
    m = members.size
    empty = np.zeros(0, np.int64)
    if m == 0:
        return empty, empty, empty
    per = target // 2 if symmetric else target
    assert not symmetric or target % 2 == 0
    need = lambda t: np.where(t == 0, 1, 2 * t + 1 if symmetric else t + 1)
    count = m // int(need(np.array(min(t_choices)))) + 1
    t = rng.choice(np.asarray(t_choices, np.int64), size=count)
    g = need(t) + rng.integers(0, 4, size=count)
    ends = np.cumsum(g)
    k = int(np.searchsorted(ends, m, side="right"))
    assert k >= 1, "the set is smaller than one group"
    t, g = t[:k].copy(), g[:k].copy()
    g[-1] += m - int(ends[k - 1])                                    # the last group takes the rest
    start = np.cumsum(g) - g
    grp = np.repeat(np.arange(k), g)
    q = np.arange(m) - start[grp]
    wstart = np.cumsum(t) - t
    total = int(t.sum())
    if total == 0:
        assert per == 0
        return empty, empty, empty
    w = rng.integers(1, 4, size=total) * rng.choice([-1, 1], size=total)
    has = t > 0
    assert per == 0 or has.all()
    last = (wstart + t - 1)[has]
    w[last] = 0
    w[last] = per - np.add.reduceat(w, wstart[has])
    zero = w[last] == 0
    if zero.any():                                                   # move the first weight by 1 (2 from -1): no zero weight
        assert np.all(t[has][zero] >= 2)
        first = wstart[has][zero]
        moved = np.where(w[first] == -1, 1, w[first] + 1)
        w[last[zero]] = w[first] - moved
        w[first] = moved
    assert np.all(w != 0) and np.array_equal(np.add.reduceat(w, wstart[has]), np.full(int(has.sum()), per))
    tr = t[grp]
    pos = np.repeat(np.arange(m), tr)
    kk = np.arange(pos.size) - np.repeat(np.cumsum(tr) - tr, tr) + 1          # 1..t within a row
    gg, st, qq = g[grp][pos], start[grp][pos], q[pos]
    wt = w[wstart[grp][pos] + kk - 1]
    rows, cols = members[pos], members[st + (qq + kk) % gg]
    if not symmetric:
        return rows, cols, wt
    return np.concatenate([rows, rows]), np.concatenate([cols, members[st + (qq - kk) % gg]]), np.concatenate([wt, wt])


def two_eig_lengths(solver, L):
    """(t choices of S1, of S2) that put the average row length inside L's range of the lane rule."""
    if solver == "cg":                                               # a row holds 2 t + 1 entries
        if L == 1:
            return [1], [0, 2, 2, 2, 3]
        both = list(range(66, 91)) if L == 64 else list(range(L, 2 * L))
        return both, both
    if L == 1:                                                       # a row holds t + 1 entries
        return [1, 2, 3], [1, 2, 3]
    both = list(range(130, 181)) if L == 64 else list(range(2 * L, 4 * L - 1))
    return both, both


def two_eig_sets(solver, n):
    """(rows of S1, rows of S2, diagonal-only rows, their |b|) that meet the weight condition at this n."""
    if solver == "cg":
        f = n % 3
        n2 = (n - 19 * f) // 3
        n1 = 2 * (n2 + 9 * f)
        fill_b = 3
    else:
        f = n % 4
        n2 = n // 4
        n1 = 3 * n2
        fill_b = 0
    assert n1 > 0 and n2 > 0 and n1 + n2 + f == n
    return n1, n2, f, fill_b


_two_eig_cache = {}


def _two_eig_structure(solver, n, L):
    """What the scaled and the unscaled system of one (solver, n, L) share; the last two are kept."""
    key = (solver, n, L)
    if key in _two_eig_cache:
        return _two_eig_cache[key]
    symmetric = solver == "cg"
    d = TWO_EIG_D
    rng = np.random.default_rng([n, L, int(symmetric)])
    n1, n2, f, fill_b = two_eig_sets(solver, n)
    perm = rng.permutation(n)
    for row, slot in ((n - 1, 0), (n - 2, n1)):                      # the last row in S1, the one before it in S2: a last
        at = int(np.flatnonzero(perm == row)[0])                     # trip of two rows or more still holds both sets
        perm[at], perm[slot] = perm[slot], perm[at]
    S1, S2 = perm[:n1], perm[n1:n1 + n2]
    sets = np.zeros(n, np.int64)
    sets[S1], sets[S2] = 1, 2
    t1, t2 = two_eig_lengths(solver, L)
    r1, c1, v1 = _circulant_rows(rng, S1, t1, -3 * d // 4, symmetric)
    r2, c2, v2 = _circulant_rows(rng, S2, t2, 0 if symmetric else -5 * d // 4, symmetric)
    idx = np.arange(n)
    rows, cols = np.concatenate([r1, r2, idx]), np.concatenate([c1, c2, idx])
    vals = np.concatenate([v1, v2, np.full(n, d, np.int64)])
    order = np.lexsort((rng.random(rows.size), rows))                # storage order inside a row is drawn
    rows, cols, vals = rows[order], cols[order], vals[order]
    sign = rng.choice([-1, 1], size=n)
    vals = vals * sign[rows] * sign[cols]
    if symmetric:
        e = rng.integers(-1, 3, size=n)
    else:
        e, k1 = np.zeros(n, np.int64), n2 // 2
        e[S1[:3 * k1]] = 1
        e[S2[:k1]] = 1
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    assert lanes_for(int(rp[-1]), n) == L, (solver, n, L, int(rp[-1]) / n)
    b_u = np.where(sets == 0, fill_b, 1).astype(np.float64) * sign + 0.0       # + 0.0: a zero entry is +0
    while len(_two_eig_cache) >= 2:
        _two_eig_cache.pop(next(iter(_two_eig_cache)))
    _two_eig_cache[key] = (rp, rows, cols.astype(np.int32), vals, sets, e, b_u)
    return _two_eig_cache[key]


def two_eig_system(solver, n, L, scaled):
    """dict(n, L, rp, ci, va, b, x1, x2, rel1, sets, e, diag, symmetric): the system above for solver "cg" or "bicgstab";
    x1 / x2 the iterates after one and two steps from x0 = 0 (x2 == A^-1 b), rel1 = ||r1|| / ||b|| rounded to float32
    from fp64, sets[i] = 1, 2 (0: a diagonal-only row), e the exponents of T (zeros when not scaled), diag the stored
    diagonal d T^2."""
    symmetric = solver == "cg"
    rp, rows, ci, vals, sets, e, b_u = _two_eig_structure(solver, n, L)
    d, lam = TWO_EIG_D, TWO_EIG_D / 4
    if scaled:
        va = np.ldexp(vals.astype(np.float64), e[rows] + e[ci]).astype(np.float32)
    else:
        va, e = vals.astype(np.float32), np.zeros(n, np.int64)
    T = np.ldexp(1.0, e)
    in1 = sets == 1
    if symmetric:
        x1_u, x2_u = b_u / (2 * lam), np.where(in1, b_u / lam, b_u / (4 * lam))
        res_u = np.where(in1, b_u / 2, -b_u)
    else:
        x1_u, x2_u = np.where(in1, 2.5, 0.5) * b_u / lam, np.where(in1, 1.0, -1.0) * b_u / lam
        res_u = np.where(in1, -1.5, 1.5) * b_u
    x1_u, x2_u = x1_u + 0.0, x2_u + 0.0                              # -0 -> +0: the solvers never produce a -0 from b = +0
    b64, res = b_u * T, res_u * T
    rel1 = np.float32(np.sqrt(np.sum(res * res)) / np.sqrt(np.sum(b64 * b64)))
    return dict(solver=solver, n=n, L=L, scaled=bool(scaled), symmetric=symmetric, rp=rp, ci=ci, va=va,
                b=b64.astype(np.float32), x1=(x1_u / T).astype(np.float32), x2=(x2_u / T).astype(np.float32), rel1=rel1,
                sets=sets, e=e, diag=np.ldexp(float(d), 2 * e).astype(np.float32))


def diagonal_csr(values):
    """(row_ptrs, cols, vals) of diag(values): the IC factor diag(sqrt(A_ii)) and the LU factor (L = I, U = diag(A_ii))."""
    n = len(values)
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(values, np.float32)


def init_solution(system):
    """(x*, b = A x*) for the exact init test on an UNSCALED system: x* integers in [-8, 8]."""
    assert not system["scaled"]
    x_star = np.random.default_rng(system["n"]).integers(-8, 9, size=system["n"]).astype(np.float32)
    check_exact(system["rp"], system["ci"], system["va"], x_star)
    return x_star, exact_reference(system["rp"], system["ci"], system["va"], x_star)


# ------------------------------------------------------------------------------------------ two wide levels
# sptrsv_kernel<L, ORDERED> past its grid cap: a triangular integer system of exactly two levels, each wider than the
# row_trip(L) rows one trip of 2048 workgroups takes.  Half the rows hold their diagonal entry only; every row of the
# other half holds 1..2 L + 2 entries at random rows of the first half, so a row of either trip reads x of both.
SPTRSV_TRIP_LANES = (1, 8)


def two_level_triangle(L, uplo, unit):
    """dict(n, rp, ci, va, b, x): n = 2 row_trip(L) + 2 (256 / L) + 2; values +-1..8, the diagonal a power of two
    (the stored 3 that a UNIT solve ignores), x integers in [-100, 100], b = T x in integers."""
    half = row_trip(L) + 256 // L + 1
    n = 2 * half
    rng = np.random.default_rng([L, uplo, unit])
    lens = rng.integers(1, 2 * L + 3, size=half)
    rows = np.repeat(np.arange(half, n), lens)
    cols = rng.integers(0, half, size=rows.size)
    vals = rng.integers(1, 9, size=rows.size) * rng.choice([-1, 1], size=rows.size)
    keys = np.unique(rows * n + cols, return_index=True)[1]          # distinct columns inside a row
    rows, cols, vals = rows[keys], cols[keys], vals[keys]
    diag = np.full(n, 3, np.int64) if unit else 1 << rng.integers(0, 4, size=n)
    idx = np.arange(n)
    rows, cols, vals = np.concatenate([rows, idx]), np.concatenate([cols, idx]), np.concatenate([vals, diag])
    x = rng.integers(-100, 101, size=n)
    if uplo == 1:                                                    # mirror: row i -> n - 1 - i
        rows, cols, x = n - 1 - rows, n - 1 - cols, x[::-1].copy()
    order = np.lexsort((rng.random(rows.size), rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    eff = np.where((rows == cols) & bool(unit), 1, vals)
    prod = eff * x[cols]
    b = np.bincount(rows, weights=prod.astype(np.float64), minlength=n).astype(np.int64)
    assert int(np.bincount(rows, weights=np.abs(prod).astype(np.float64), minlength=n).max()) < EXACT_LIMIT
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return dict(n=n, half=half, L=L, uplo=uplo, unit=unit, rp=rp, ci=cols.astype(np.int32), va=vals.astype(np.float32),
                b=b.astype(np.float32), x=x.astype(np.float32))


# ------------------------------------------------------------------------------------------ one-hot Lanczos systems
# eigs_sym (csrc/eigs.hip) held to the bit up to its first close: the symmetric counterpart of the one-hot Krylov
# systems.  A = D + B + B^T with B[i, (i - s) mod n] = beta_i, every stored value +- a power of two (|d| 1 or 2, |beta|
# 1/2, 1 or 2), the link between p and (p - s) mod n removed, so that from v0 = 4 e_p the Lanczos vectors are
# v_j = sign_j e_(q_j), q_j = (p + j s) mod n, sign_0 = +1, sign_j = sign_(j-1) sgn(beta_(q_j)): A v_j holds at most three
# non-zeros, one per row, h1 is d_(q_j) at i = j, |beta_(q_j)| at i = j - 1 and 0.0 elsewhere (one non-zero product per
# dot product), the updated w is sign_j beta_(q_j+1) e_(q_j+1), h2 is 0.0, w.w = beta^2 and 1 / |beta| a power of two.
# T is the tridiagonal matrix of the walk (diagonal d_(q_j), off-diagonal |beta_(q_j+1)|) whatever the order of any
# reduction; the Ritz decomposition is a fixed sequence of fp64 operations, the same on the host and on the device; and
# a rotation y_i = sum_l C[i, l] v_l has one non-zero product per element.  So the values and vectors of a run that
# finishes at its FIRST close are predictable from T alone.  The recomputed residuals are not claimed: a row of A y_i sums
# up to three rounded fp32 products in an order the lane count decides.  After a thick restart the basis vectors are
# dense on the walk, dot products sum many terms of mixed exponent, and the bits depend on the order (measured in
# tests/test_exact_data.py): such runs are held to eigs_cases' bounds, with the exact claim that nothing leaves the walk.
LANCZOS_START = 4.0                  # v0 = 2^2 e_p


def lanczos_onehot_system(n, p, s, steps, seed, cut=None):
    """dict(n, rp, ci, va, v0, walk, d, beta, sign, cut): the system above.  `walk` holds q_0..q_steps, asserted
    distinct; row i stores d_i at column i, beta_i at column (i - s) mod n and beta_(i+s) at column (i + s) mod n, in an
    order drawn per row; both entries linking p with (p - s) mod n are removed, and with cut = j both entries linking
    q_j with q_j+1 as well (step j then finds w == 0: an invariant space of j + 1 columns).  sign[j] is v_j's sign."""
    assert 0 <= p < n and 0 < s < n and steps + 1 <= n and (2 * s) % n != 0
    rng = np.random.default_rng(seed)
    walk = (p + s * np.arange(steps + 1, dtype=np.int64)) % n
    assert np.unique(walk).size == steps + 1, "the walk revisits a position"
    assert (p - s) % n not in set(walk.tolist())
    d = np.ldexp(rng.choice([-1.0, 1.0], size=n), rng.integers(0, 2, size=n)).astype(np.float32)
    beta = np.ldexp(rng.choice([-1.0, 1.0], size=n), rng.integers(-1, 2, size=n)).astype(np.float32)
    idx = np.arange(n, dtype=np.int64)
    rows = np.concatenate([idx, idx, (idx - s) % n])               # D, B, B^T
    cols = np.concatenate([idx, (idx - s) % n, idx])
    vals = np.concatenate([d, beta, beta])
    keep = np.ones(3 * n, bool)
    for i in [p] + ([int(walk[cut + 1])] if cut is not None else []):      # the link beta_i between i and (i - s) mod n
        keep[n + i] = keep[2 * n + i] = False
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((rng.random(rows.size), rows))              # storage order inside a row is drawn
    rows, cols, vals = rows[order], cols[order], vals[order]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    v0 = np.zeros(n, np.float32)
    v0[p] = LANCZOS_START
    sign = np.cumprod(np.concatenate([[1.0], np.sign(beta[walk[1:]])])).astype(np.float32)
    return dict(n=n, s=s, rp=rp, ci=cols.astype(np.int32), va=vals.astype(np.float32), v0=v0, walk=walk, d=d, beta=beta,
                sign=sign, cut=cut)


def lanczos_onehot_compact(system):
    """(m, rp, ci, va, v0) of the system restricted to its walk, in walk order: row j is row q_j with its entries in
    storage order, those whose column lies off the walk dropped (every vector is 0 there from start to end)."""
    walk = system["walk"]
    at = {int(q): j for j, q in enumerate(walk)}
    rp, ci, va = system["rp"], system["ci"], system["va"]
    c_rp, c_ci, c_va = [0], [], []
    for q in walk:
        for e in range(int(rp[q]), int(rp[q + 1])):
            if int(ci[e]) in at:
                c_ci.append(at[int(ci[e])])
                c_va.append(va[e])
        c_rp.append(len(c_ci))
    return (walk.size, np.array(c_rp, np.int32), np.array(c_ci, np.int32), np.array(c_va, np.float32),
            system["v0"][walk].copy())


def lanczos_onehot_reference(system, k, which, m, max_iterations, spmv=None):
    """eigs_cases.restate on the walk positions only at tolerance 0, the vectors scattered back: restate's dict.
    tests/test_exact_data.py shows that it equals restate on the whole system in every field at small n.  The walk has
    to be longer than the basis (restate clips m to the order of the system it is given)."""
    import eigs_cases as ec
    order, rp, ci, va, v0 = lanczos_onehot_compact(system)
    assert order > m and order > max_iterations
    out = ec.restate(order, rp, ci, va, k, which, m, tol=0.0, max_iter=max_iterations, v0=v0,
                     **({} if spmv is None else {"spmv": spmv}))
    vectors = np.zeros((k, system["n"]), np.float32)
    vectors[:, system["walk"]] = out["vectors"]
    return dict(out, vectors=vectors)


def lanczos_onehot_tridiagonal(system, c):
    """T after c steps of the first cycle: diagonal d_(q_j), off-diagonal |beta_(q_j+1)|, in fp64."""
    walk = system["walk"]
    assert system["cut"] is None or c <= system["cut"] + 1
    T = np.diag(system["d"][walk[:c]].astype(np.float64))
    off = np.abs(system["beta"][walk[1:c]].astype(np.float64))
    T[np.arange(c - 1), np.arange(1, c)] = off
    T[np.arange(1, c), np.arange(c - 1)] = off
    return T


def lanczos_onehot_prediction(system, k, which, c):
    """(values, vectors k x n) of a run that finishes at its first close with c columns, from T alone: values[i] =
    fp32(theta_i), vector i = fp32(S[i, l]) sign_l at q_l for l < c and 0 elsewhere (+ 0.0: a rotation's sum starts
    at +0, so a zero coefficient gives +0 whatever its sign); NaN / zero rows from min(k, c) on."""
    import eigs_cases as ec
    values, S, _ = ec.jacobi(lanczos_onehot_tridiagonal(system, c))
    theta, S = ec.sort_ritz(values, S, which)
    found = min(k, c)
    out_values = np.full(k, np.nan, np.float32)
    out_values[:found] = theta[:found].astype(np.float32)
    vectors = np.zeros((k, system["n"]), np.float32)
    vectors[:found, system["walk"][:c]] = (S[:found].astype(np.float32) * system["sign"][:c]) + np.float32(0.0)
    return out_values, vectors


def lanczos_runs(c):
    """[(k, m, c)] for a first close with c columns: k in {1, min(c, 32), min(c + 2, 32)}.  eigs.h admits k < m only, so
    k < c runs at the basis m = c (the cycle closes on j + 1 == m) and k >= c at the smallest basis that admits k,
    m = k + 1, with max_iterations = c (the cycle closes on its budget): the same c columns either way."""
    return [(k, c if k < c else k + 1, c) for k in sorted({1, min(c, 32), min(c + 2, 32)})]


LANCZOS_BASIS_EDGES = (1, 2, 7, 8, 9, 16, 17, 63, 64)


def _lanczos_cases():
    cases = {}

    def add(name, geometry, runs, visits=(), chunks=(), cut=None, nan_step=None):
        g = ONEHOT_CASES[geometry]
        steps = max(max(m, c) for _, m, c in runs) + 1
        cases[name] = dict(name=name, n=g["n"], p=g["p"], s=g["s"], steps=steps, runs=tuple(runs), visits=tuple(visits),
                           chunks=tuple(chunks), cut=cut, nan_step=nan_step, seed=len(cases) + 117)

    # the basis edges at n = 4103 (3 mod 4): one, two, a group of eight less one, full, plus one, two groups, the cap
    for c in LANCZOS_BASIS_EDGES:
        add("basis_%d" % c, "restart_9", lanczos_runs(c),
            visits=(4100, 1023) if c < 16 else (4100, 4101, 4102, 0, 1023, 1024))
    # the host closes on the budget, one column before j + 1 == m
    add("budget_before_basis", "restart_9", [(1, 9, 8), (8, 9, 8)], visits=(4100, 1023))
    # vector tails at n mod 4 = 1 and 2 (n mod 4 = 3: basis_16 and up)
    add("tail_n3077", "tail_n3077", lanczos_runs(16), visits=(3074, 3075, 3076, 0, 1023, 1024))
    add("tail_n3074", "tail_n3074", lanczos_runs(16), visits=(3071, 3072, 3073, 0, 1023, 1024))
    # the large geometries keep m <= 9: k = 1 and 8 at c = m = 9, and k = 5 > c = 3 (zero rows past every edge)
    large = [(1, 9, 9), (8, 9, 9), (5, 9, 3)]
    add("fold_second_trip", "fold_second_trip", large, visits=(5, 65545, 131085), chunks=(0, 64, 128))
    add("grid_second_trip", "grid_second_trip", large, visits=(261125, 262148, 263171, 264194),
        chunks=(254, 255, 256, 257, 258, 0))
    add("rows_second_trip", "rows_second_trip", large, visits=(523268, 524291, 525314, 1022))
    # both entries between q_5 and q_6 removed: six columns, then w == 0; the host learns of the close one step late
    add("invariant_mid_cycle", "restart_9", [(1, 9, 19), (6, 9, 19), (8, 9, 19)], visits=(4100, 1023, 4101), cut=5)
    # the diagonal entry of row q_2 is NaN: NaN * 0 is NaN, so the first step is NOT_FINITE; eigs_fill_failed on
    # 525 315 rows
    add("nan_on_the_walk", "rows_second_trip", [(3, 9, 9)], visits=(523268, 524291, 525314), nan_step=2)
    return cases


LANCZOS_CASES = _lanczos_cases()
LANCZOS_NAMES = list(LANCZOS_CASES)
# thick restarts (no bit claim): (geometry, k, m), run for 2 m + 1 steps
LANCZOS_RESTART_CASES = [("grid_second_trip", 2, 8), ("grid_second_trip", 2, 9), ("rows_second_trip", 2, 8),
                         ("rows_second_trip", 2, 9), ("restart_9", 4, 20)]
_lanczos_cache = {}


def lanczos_case(name):
    """(case, system) of one LANCZOS_CASES member; the system is built once.  A nan_step case carries the finite
    system; lanczos_nan_values gives the stored values with the NaN."""
    if name not in _lanczos_cache:
        c = LANCZOS_CASES[name]
        _lanczos_cache[name] = (c, lanczos_onehot_system(c["n"], c["p"], c["s"], c["steps"], c["seed"], c["cut"]))
    return _lanczos_cache[name]


def lanczos_nan_values(case, system):
    """The stored values with the diagonal entry of row q_(nan_step) replaced by NaN."""
    q = int(system["walk"][case["nan_step"]])
    va = system["va"].copy()
    lo, hi = int(system["rp"][q]), int(system["rp"][q + 1])
    va[lo + int(np.flatnonzero(system["ci"][lo:hi] == q)[0])] = np.nan
    return va


def lanczos_restart_case(geometry, k, m):
    """(system, max_iterations) of one LANCZOS_RESTART_CASES member: 2 m + 1 steps, a walk of 2 m + 3 positions."""
    key = ("restart", geometry, k, m)
    if key not in _lanczos_cache:
        g = ONEHOT_CASES[geometry]
        seed = 400 + LANCZOS_RESTART_CASES.index((geometry, k, m))
        _lanczos_cache[key] = (lanczos_onehot_system(g["n"], g["p"], g["s"], 2 * m + 2, seed), 2 * m + 1)
    return _lanczos_cache[key]


def lanczos_lambda_max(system):
    """max |lambda| of the walk's tridiagonal matrix (the compact system, dense; asserted symmetric and tridiagonal)"""
    m, rp, ci, va, _ = lanczos_onehot_compact(system)
    D = np.zeros((m, m))
    np.add.at(D, (np.repeat(np.arange(m), np.diff(rp)), ci), va.astype(np.float64))
    assert np.array_equal(D, D.T) and not np.triu(D, 2).any()
    return float(np.max(np.abs(np.linalg.eigvalsh(D))))


# ------------------------------------------------------------------------------------------ Lanczos, first step
LANCZOS_STEP_K = 5                            # 1024 rows, as GMRES_STEP_K
LANCZOS_STEP_VALUES = 3                       # num_values of the run: one pair found, two NaN / zero rows
LANCZOS_SEEDS = 20                            # seeds tried per system before the construction gives up


def lanczos_first_step(rp, ci, va, v0, k):
    """What eigs_sym returns after ONE Lanczos step (max_iterations 1, tolerance 0, num_values > 1) under eigs.h's rules,
    for an integer matrix and a +-1 / 0 start vector with 4^k non-zeros (pm_one_rhs).  beta_0 = 2^k and v_0 = v0 / 2^k
    exactly; w = A v0 / 2^k holds integers over 2^k; h1 = v0.A v0 / 4^k is an exact fp32 value; fmaf(-h1, v_0, w) =
    (4^k (A v0)_i - v0_i (v0.A v0)) / 8^k with a numerator below 2^24: exact; h2 == 0; T = [h1], so theta = h1, S = [1] and
    y_0 = v_0.  The finish: t = A y_0 = w (integers over 2^k, exact in any lane order), d = fmaf(-theta, y_0, t) the same
    exact vector as the updated w, d.d a sum of integers over 64^k that stays below 2^53: exact in fp64 in any order; the
    residual is fp32(sqrt(d.d)) given a correctly rounded fp64 square root.  beta = sqrt(w.w) = sqrt(d.d); the space is
    invariant when beta <= |h1| 2^-20.  Every claim is asserted.  Returns dict(value, vector, residual (float32),
    invariant, converged)."""
    v0 = np.asarray(v0, np.float32)
    check_exact(rp, ci, va, v0)
    b64 = v0.astype(np.int64)
    scale = 4 ** k
    assert set(np.unique(b64).tolist()) <= {-1, 0, 1} and int(np.abs(b64).sum()) == scale == int(b64 @ b64)
    ab = exact_reference(rp, ci, va, v0).astype(np.int64)                        # 2^k w
    bab = int(b64 @ ab)
    h1 = np.float32(np.float64(bab) / np.float64(scale))
    assert np.float64(h1) * scale == bab and abs(bab) < EXACT_LIMIT             # an exact fp32 value
    num = scale * ab - b64 * bab                                                 # 8^k (w after the first update)
    assert int(np.abs(num).max()) < EXACT_LIMIT                                  # ... which fp32 holds: the fmaf is exact
    assert int(b64 @ num) == 0                                                   # h2 == 0: the second update changes nothing
    dd_int = sum(int(v) * int(v) for v in num[num != 0])                         # 64^k d.d
    assert 0 <= dd_int < 2 ** 53
    beta = np.sqrt(np.float64(dd_int) / np.float64(64 ** k))
    vector = (v0.astype(np.float64) / np.float64(2 ** k)).astype(np.float32)
    assert np.array_equal(vector.astype(np.float64) * 2 ** k, v0.astype(np.float64))
    return dict(value=h1, vector=vector, residual=np.float32(beta), invariant=bool(beta <= abs(np.float64(h1)) * 2.0 ** -20),
                converged=int(beta <= 0.0), ab=ab, num=num)


def _lanczos_start(rp, ci, va, n, k, base_seed, accept):
    """(v0, first step) from the first of LANCZOS_SEEDS seeds whose +-1 / 0 vector meets lanczos_first_step's bounds and
    `accept`; a seed that fails a bound is passed over, as the construction allows."""
    for t in range(LANCZOS_SEEDS):
        v0 = pm_one_rhs(n, k, base_seed + 1000 * t)
        try:
            step = lanczos_first_step(rp, ci, va, v0, k)
        except AssertionError:
            continue
        if accept(v0, step):
            return v0, step
    raise AssertionError("no seed of %d gives an exact first step" % LANCZOS_SEEDS)


_lanczos_step_cache = {}


def lanczos_step_system(name):
    """(L, n, rp, ci, va, v0, first step) of solver_system(name, symmetric=True) with a +-1 / 0 start vector on 4^5
    rows.  L1_low is the diagonal plus one symmetric pair: its start vector is drawn until A v0 == v0 (the pair's rows
    cancel or lie outside the support), the run that ends with INVARIANT_SUBSPACE, value 1 and residual 0."""
    if name not in _lanczos_step_cache:
        L, n, rp, ci, va, _, _ = solver_system(name, symmetric=True)
        accept = (lambda v0, step: step["invariant"]) if name == "L1_low" else (lambda v0, step: not step["invariant"])
        v0, step = _lanczos_start(rp, ci, va, n, LANCZOS_STEP_K, 1500 + SOLVER_NAMES.index(name), accept)
        _lanczos_step_cache[name] = (L, n, rp, ci, va, v0, step)
    return _lanczos_step_cache[name]


LANCZOS_TRIP_LANES = (2, 8, 64)               # the row loop's second trip at L > 1
LANCZOS_TRIP_AVERAGE = {L: 3 * L for L in LANCZOS_TRIP_LANES}     # inside (2 L, 4 L]: the lane rule gives L


def lanczos_trip_system(L):
    """(n, rp, ci, va, v0, first step): integer_spd at n = LANE_SIZES[L] rows and an average of 3 L entries per row, the
    start vector drawn until its support and the non-zeros of A v0 lie on both sides of row_trip(L), the first row of
    the row loop's second trip.  k = 5 for every L (no seed had to give way to k = 4)."""
    key = ("trip", L)
    if key not in _lanczos_step_cache:
        n = LANE_SIZES[L]
        total = LANCZOS_TRIP_AVERAGE[L] * n
        n, rp, ci, va = integer_spd(n, (total - n) // 2, seed=1600 + L)
        edge = row_trip(L)

        def accept(v0, step):
            both = lambda mask: bool(mask[:edge].any() and mask[edge:].any())
            return both(v0 != 0) and both(step["ab"] != 0) and not step["invariant"]

        v0, step = _lanczos_start(rp, ci, va, n, LANCZOS_STEP_K, 1700 + L, accept)
        while len(_lanczos_step_cache) >= 20:
            _lanczos_step_cache.pop(next(iter(_lanczos_step_cache)))
        _lanczos_step_cache[key] = (n, rp, ci, va, v0, step)
    return _lanczos_step_cache[key]


LANCZOS_TILED_STEP_K = 7                      # 16 384 of the 20 011 rows of entry_point_systems


def lanczos_tiled_step_system(W):
    """(n, rp, ci, va, v0, first step): the symmetric system of entry_point_systems(W) with a +-1 / 0 start vector."""
    key = ("tiled", W)
    if key not in _lanczos_step_cache:
        n, rp, ci, va = entry_point_systems(W)[0]
        v0, step = _lanczos_start(rp, ci, va, n, LANCZOS_TILED_STEP_K, 1800 + W, lambda v0, step: not step["invariant"])
        _lanczos_step_cache[key] = (n, rp, ci, va, v0, step)
    return _lanczos_step_cache[key]
