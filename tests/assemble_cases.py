"""Matrix assembly (include/spmv/assemble.h): the restatement of the header's definition in numpy, the case
generators of tests/test_assemble_host.py and tests/test_gpu_assemble.py, and the proof that the restatement's order
is that of a plain dictionary-of-lists accumulation.

The restatement: a stable lexsort by (row, column); with COO_SUM every run of equal pairs is added left to right in
np.float32, starting from its first value, so a lone value keeps its bits; a run of two or more whose sum is a NaN
gives 0x7FC00000 (IEEE 754 leaves the NaN of an addition open, the header closes it).  With COO_KEEP every triplet is
an entry.  row_ptrs counts the entries of the rows above.

A plain module, not a conftest: imported by the two test files."""
import numpy as np

SUM, KEEP = 0, 1
MODES = (SUM, KEEP)
QUIET_NAN = np.uint32(0x7FC00000)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(words):
    return np.asarray(words, np.uint32).view(np.float32)


def assemble(num_rows, num_cols, rows, cols, vals, mode=SUM):
    """(row_ptrs, col_indices, values) of the definition."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.ascontiguousarray(vals, np.float32)
    n = rows.size
    assert cols.size == n and vals.size == n
    assert n == 0 or (rows.min() >= 0 and rows.max() < num_rows and cols.min() >= 0 and cols.max() < num_cols)
    order = np.lexsort((cols, rows))                       # stable: equal pairs keep ascending source position
    r, c = rows[order], cols[order]
    if mode == KEEP:
        head = np.ones(n, bool)
    else:
        head = np.ones(n, bool)
        head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    out_bits = bits(vals)[order][starts].copy()            # a lone value: its bits
    with np.errstate(all="ignore"):
        for o in np.flatnonzero(ends - starts > 1):
            s = vals[order[starts[o]]]
            for t in range(starts[o] + 1, ends[o]):
                s = np.float32(s + vals[order[t]])
            out_bits[o] = QUIET_NAN if np.isnan(s) else np.float32(s).reshape(1).view(np.uint32)[0]
    row_ptrs = np.zeros(num_rows + 1, np.int64)
    np.add.at(row_ptrs, r[starts] + 1, 1)
    return np.cumsum(row_ptrs).astype(np.int32), c[starts].astype(np.int32), out_bits.view(np.float32)


def by_dictionary(num_rows, num_cols, rows, cols, vals):
    """COO_SUM as A[i, j] += v in source order over a dictionary of lists, with no sort of the triplets at all."""
    cells = {}
    for p in range(len(rows)):
        cells.setdefault((int(rows[p]), int(cols[p])), []).append(p)
    vals = np.ascontiguousarray(vals, np.float32)
    row_ptrs = np.zeros(num_rows + 1, np.int32)
    out_cols, out_bits, sources = [], [], []
    with np.errstate(all="ignore"):
        for (i, j) in sorted(cells):
            places = cells[(i, j)]
            s = vals[places[0]]
            for p in places[1:]:
                s = np.float32(s + vals[p])
            word = bits(vals)[places[0]] if len(places) == 1 else (
                QUIET_NAN if np.isnan(s) else np.float32(s).reshape(1).view(np.uint32)[0])
            row_ptrs[i + 1] += 1
            out_cols.append(j)
            out_bits.append(word)
            sources.append(places)
    return (np.cumsum(row_ptrs).astype(np.int32), np.asarray(out_cols, np.int32),
            np.asarray(out_bits, np.uint32).view(np.float32), sources)


def same(got, want):
    """zero tolerance: row_ptrs, col_indices and the values' bit patterns"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


# ------------------------------------------------------------------------------------------ generators
def general_values(rng, n):
    v = (rng.standard_normal(n) * 10.0).astype(np.float32)
    v[v == 0.0] = 1.0
    return v


def uniform(num_rows, num_cols, n, seed):
    rng = np.random.default_rng(seed)
    return (num_rows, num_cols, rng.integers(0, num_rows, n).astype(np.int32),
            rng.integers(0, num_cols, n).astype(np.int32), general_values(rng, n))


def shuffled(case, seed):
    num_rows, num_cols, rows, cols, vals = case
    p = np.random.default_rng(seed).permutation(len(rows))
    return num_rows, num_cols, rows[p], cols[p], vals[p]


def with_extremes(num_rows, num_cols, n, seed):
    """uniform, with the first and the last cell of the matrix among the triplets (twice each)"""
    num_rows, num_cols, rows, cols, vals = uniform(num_rows, num_cols, n, seed)
    rows[:4] = (0, num_rows - 1, num_rows - 1, 0)
    cols[:4] = (0, num_cols - 1, num_cols - 1, 0)
    return shuffled((num_rows, num_cols, rows, cols, vals), seed + 1)


def top_digit_only(n):
    """one column, rows k << 16 for k < 16: a 20-bit key whose digits 0 and 1 never differ"""
    rng = np.random.default_rng(11)
    rows = (rng.integers(0, 16, n) << 16).astype(np.int32)
    return (15 << 16) + 1, 1, rows, np.zeros(n, np.int32), general_values(rng, n)


def all_equal(n):
    rng = np.random.default_rng(12)
    return 9, 9, np.full(n, 5, np.int32), np.full(n, 7, np.int32), general_values(rng, n)


def run_across(slot, length=3, tail=21, seed=13):
    """one row; in sorted order a run of `length` equal columns begins at slot `slot`: `slot` distinct columns come
    before it and `tail` after it"""
    cols = np.concatenate([np.arange(slot), np.full(length, slot), slot + 1 + np.arange(tail)]).astype(np.int32)
    rng = np.random.default_rng(seed)
    case = (1, int(cols.max()) + 1, np.zeros(cols.size, np.int32), cols, general_values(rng, cols.size))
    return shuffled(case, seed + 1)


def three_keys(n):
    rng = np.random.default_rng(14)
    pick = rng.integers(0, 3, n)
    rows = np.asarray([2, 2, 40], np.int32)[pick]
    cols = np.asarray([3, 17, 0], np.int32)[pick]
    return 50, 20, rows, cols, general_values(rng, n)


def cancelling_runs(keys, seed=15):
    """every run holds 1e8, 1 and -1e8 in some source order: (1e8 + 1) - 1e8 = 0 but (1e8 - 1e8) + 1 = 1"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(rng.integers(0, 40, keys), 3).astype(np.int32)
    cols = np.repeat(rng.integers(0, 70, keys), 3).astype(np.int32)
    vals = np.tile(np.asarray([1e8, 1.0, -1e8], np.float32), keys)
    return shuffled((40, 70, rows, cols, vals), seed + 1)


def special_values():
    """(row, column, bit patterns in source order) per run"""
    runs = [
        (0, 0, [0x80000000]),                                  # -0.0 alone
        (0, 1, [0x7FC12345]),                                  # a quiet NaN with a payload alone
        (0, 2, [0xFFC00001]),                                  # a negative one
        (0, 3, [0x7F800001]),                                  # a signalling NaN alone: copied, never added
        (1, 0, [0x7F800000, 0xFF800000]),                      # +inf and -inf in one run
        (1, 1, [0xFF800000, 0x3F800000, 0x7F800000]),
        (1, 2, [0x7F800000, 0x7F800000]),                      # stays +inf
        (2, 0, [0x00000001, 0x00000001, 0x00000003]),          # subnormals: 5 * 2^-149
        (2, 1, [0x007FFFFF, 0x00000001]),                      # the largest subnormal + the smallest: the smallest normal
        (2, 2, [0x80000002, 0x00000001]),
        (3, 0, [0x3FC00000, 0xBFC00000]),                      # 1.5 - 1.5: an explicit +0
        (3, 1, [0x80000000, 0x80000000]),                      # -0 + -0 = -0
        (3, 2, [0x80000000, 0x00000000]),                      # -0 + +0 = +0
        (3, 3, [0x00000000]),                                  # an explicit zero alone
        (4, 4, [0x7FC12345, 0x3F800000]),                      # a NaN inside a run: the one spelling
        (5, 0, [0x4CBEBC20, 0x3F800000, 0xCCBEBC20]),          # 1e8, 1, -1e8
    ]
    rows = np.concatenate([[r] * len(w) for r, _, w in runs]).astype(np.int32)
    cols = np.concatenate([[c] * len(w) for _, c, w in runs]).astype(np.int32)
    vals = from_bits(np.concatenate([w for _, _, w in runs]))
    # an order that keeps every run's source order: a stable sort by a random label per run would not interleave, so
    # interleave by hand: round-robin over the runs
    position = np.concatenate([np.arange(len(w)) for _, _, w in runs])
    order = np.argsort(position, kind="stable")
    return 7, 6, rows[order], cols[order], vals[order]


def sorted_case(case, reverse=False):
    num_rows, num_cols, rows, cols, vals = case
    order = np.lexsort((cols, rows))
    if reverse:
        order = order[::-1]
    return num_rows, num_cols, rows[order], cols[order], vals[order]


def tile_edge_sizes(T):
    """label -> n; 17T + 3 entries make 18 tiles, whose 256 * 18 digit counts need a second scan level"""
    sizes = {str(n): n for n in (0, 1, 63, 64, 65, 255, 256, 257)}
    sizes.update({"T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1, "17T+3": 17 * T + 3})
    return sizes


def cases(T):
    """name -> () -> (num_rows, num_cols, rows, cols, vals); T is CooResult.tile_entries"""
    out = {}
    for label, n in tile_edge_sizes(T).items():
        out["n=" + label] = lambda n=n: uniform(700, 900, n, 100 + n % 97)
    base = lambda: uniform(50, 60, 2 * T + 5, 21)
    out.update({
        "key 32 bits": lambda: with_extremes(1 << 16, 1 << 16, 3000, 31),
        "key 33 bits": lambda: with_extremes(1 << 16, (1 << 16) + 1, 3000, 32),
        "key 48 bits": lambda: with_extremes((1 << 16) + 1, (1 << 31) - 1, 3000, 33),
        "top digit only": lambda: top_digit_only(1000),
        "all equal": lambda: all_equal(17 * T + 3),
        "sorted": lambda: sorted_case(base()),
        "reverse sorted": lambda: sorted_case(base(), reverse=True),
        "shuffled": base,
        "three keys": lambda: three_keys(1000),
        "run from slot T-1 to T+1": lambda: run_across(T - 1),
        "run from slot 63": lambda: run_across(63),
        "1 x 1": lambda: (1, 1, np.zeros(5, np.int32), np.zeros(5, np.int32), general_values(np.random.default_rng(41), 5)),
        "one row": lambda: uniform(1, 5000, 3000, 42),
        "one column": lambda: uniform(5000, 1, 3000, 43),
        "empty first and last rows": lambda: (lambda c: (10, c[1], c[2] + 3, c[3], c[4]))(uniform(4, 30, 200, 44)),
        "1000 empty rows": lambda: (1002, 3, np.asarray([1001, 0], np.int32), np.asarray([2, 0], np.int32),
                                    np.asarray([2.5, -1.25], np.float32)),
        "1e8, 1, -1e8": lambda: cancelling_runs(400),
        "special values": special_values,
    })
    return out


# passes the device sort runs: the 8-bit digits of the key in which two triplets differ
def expected_passes(num_rows, num_cols, rows, cols):
    if len(rows) == 0:
        return 0
    col_bits = max(int(num_cols) - 1, 0).bit_length()
    keys = (np.asarray(rows, np.uint64) << np.uint64(col_bits)) | np.asarray(cols, np.uint64)
    diff = int(np.bitwise_or.reduce(keys ^ keys[0]))
    return sum(1 for d in range(8) if (diff >> (8 * d)) & 255)


# ------------------------------------------------------------------------------------------ Q1 grid
def q1_grid(nodes_per_side, coefficient=None, seed=51):
    """Element matrices of the Q1 (bilinear) Laplacian on a square grid: 16 contributions per element, every shared
    node repeated.  coefficient: one positive float per element (default: random in [1, 2)).  Returns (n, rows, cols,
    vals): the stiffness matrix of every element plus its mass matrix, which makes the assembled matrix positive
    definite without boundary conditions."""
    m = nodes_per_side
    elements = (m - 1) * (m - 1)
    rng = np.random.default_rng(seed)
    if coefficient is None:
        coefficient = (1.0 + rng.random(elements)).astype(np.float32)
    k_local = np.asarray([[4, -1, -2, -1], [-1, 4, -1, -2], [-2, -1, 4, -1], [-1, -2, -1, 4]], np.float32) / 6.0
    m_local = np.asarray([[4, 2, 1, 2], [2, 4, 2, 1], [1, 2, 4, 2], [2, 1, 2, 4]], np.float32) / 36.0
    local = (k_local + m_local).astype(np.float32)
    ex, ey = np.meshgrid(np.arange(m - 1), np.arange(m - 1), indexing="ij")
    ex, ey = ex.ravel(), ey.ravel()
    corners = np.stack([ex * m + ey, (ex + 1) * m + ey, (ex + 1) * m + ey + 1, ex * m + ey + 1], axis=1)   # [e, 4]
    rows = np.repeat(corners, 4, axis=1).reshape(-1).astype(np.int32)
    cols = np.tile(corners, (1, 4)).reshape(-1).astype(np.int32)
    vals = (np.asarray(coefficient, np.float32)[:, None] * local.reshape(1, 16)).astype(np.float32).reshape(-1)
    return m * m, rows, cols, vals
