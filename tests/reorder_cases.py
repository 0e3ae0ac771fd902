"""The rules of include/spmv/reorder.h restated in numpy / plain Python, rule for rule, and the small graphs the
reordering tests share (test_reorder_host.py, test_gpu_reorder.py).

* fmix32, priority: the vertex priority (fmix32(i ^ seed), i), larger first.
* color: greedy first-fit in descending priority, with the synchronous round count round(v) = 1 + the largest round
  of v's higher-priority neighbours.  color_by_rounds: the same colouring reached the other way, as the synchronous
  Jones-Plassmann iteration (every uncoloured vertex whose higher-priority neighbours were all coloured BEFORE the
  round colours in it); the two must agree in colours and in rounds.
* ordering: the vertices sorted by (colour, index).
* permute: B = P A Q^T with rows sorted by new column, equal columns in storage order.
* graphs: complete, star, path, upper_bidiagonal, diagonal_only, messy, with_row_lengths, and the library's generators
  under the names the tests use.
Every matrix is (n, row_ptrs int32, col_indices int32, values float32); rectangular ones (rows, cols, rp, ci, va).
"""
import importlib

import numpy as np

spd = importlib.import_module("gpu-spmv_amd.spd")
nonsym = importlib.import_module("gpu-spmv_amd.nonsym")

GOLDEN = "reorder_restate.json"
MASK = 0xFFFFFFFF


def fmix32(h):
    h &= MASK
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & MASK
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & MASK
    h ^= h >> 16
    return h


def priority(i, seed=0):
    return (fmix32(i ^ seed), i)


def neighbours(n, rp, ci, symmetric_pattern=0):
    """per vertex the set of vertices it looks at: the columns of its row, and with symmetric_pattern = 0 also the
    rows that store it; never itself"""
    adj = [set() for _ in range(n)]
    for v in range(n):
        for j in range(rp[v], rp[v + 1]):
            u = int(ci[j])
            if u != v:
                adj[v].add(u)
                if not symmetric_pattern:
                    adj[u].add(v)
    return adj


def color(n, rp, ci, seed=0, symmetric_pattern=0):
    """(colors int32[n], num_colors, synchronous rounds)"""
    adj = neighbours(n, rp, ci, symmetric_pattern)
    colors = np.full(n, -1, np.int32)
    rounds = np.zeros(n, np.int64)
    for v in sorted(range(n), key=lambda i: priority(i, seed), reverse=True):
        higher = [u for u in adj[v] if priority(u, seed) > priority(v, seed)]
        held = {int(colors[u]) for u in higher}
        c = 0
        while c in held:
            c += 1
        colors[v] = c
        rounds[v] = 1 + max((rounds[u] for u in higher), default=0)
    return colors, (int(colors.max()) + 1 if n else 0), (int(rounds.max()) if n else 0)


def color_by_rounds(n, rp, ci, seed=0, symmetric_pattern=0):
    """the synchronous Jones-Plassmann iteration; (colors, num_colors, rounds)"""
    adj = neighbours(n, rp, ci, symmetric_pattern)
    higher = [[u for u in adj[v] if priority(u, seed) > priority(v, seed)] for v in range(n)]
    colors = np.full(n, -1, np.int32)
    left = list(range(n))
    rounds = 0
    while left:
        before = colors.copy()
        ready = [v for v in left if all(before[u] >= 0 for u in higher[v])]
        assert ready                                     # the highest-priority uncoloured vertex always is
        for v in ready:
            held = {int(before[u]) for u in higher[v]}
            c = 0
            while c in held:
                c += 1
            colors[v] = c
        done = set(ready)
        left = [v for v in left if v not in done]
        rounds += 1
    return colors, (int(colors.max()) + 1 if n else 0), rounds


def is_proper(n, rp, ci, colors):
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    off = rows != ci
    return bool(np.all(colors[rows[off]] != colors[np.asarray(ci)[off]]))


def structurally_symmetric(n, rp, ci):
    stored = {(i, int(ci[j])) for i in range(n) for j in range(rp[i], rp[i + 1])}
    return all((c, r) in stored for r, c in stored)


def ordering(colors, num_colors):
    """(perm, inverse, color_ptr): perm[new] = old, vertices by (colour, index)"""
    colors = np.asarray(colors, np.int64)
    perm = np.lexsort((np.arange(colors.size), colors)).astype(np.int32)
    inverse = np.empty(colors.size, np.int32)
    inverse[perm] = np.arange(colors.size, dtype=np.int32)
    color_ptr = np.concatenate([[0], np.cumsum(np.bincount(colors, minlength=num_colors))]).astype(np.int32)
    return perm, inverse, color_ptr


def permute(rows, cols, rp, ci, va, row_perm=None, col_inverse=None):
    """(row_ptrs, col_indices, values) of B = P A Q^T, rows sorted by new column, equal columns in storage order"""
    row_perm = np.arange(rows) if row_perm is None else np.asarray(row_perm)
    col_inverse = np.arange(cols) if col_inverse is None else np.asarray(col_inverse)
    new_rp, new_ci, new_va = [0], [], []
    for i in range(rows):
        src = int(row_perm[i])
        entries = [(int(col_inverse[ci[j]]), j) for j in range(rp[src], rp[src + 1])]
        entries.sort()                                   # positions are distinct: (new column, position)
        new_ci += [c for c, _ in entries]
        new_va += [va[j] for _, j in entries]
        new_rp.append(len(new_ci))
    return (np.asarray(new_rp, np.int32), np.asarray(new_ci, np.int32).reshape(-1),
            np.asarray(new_va, np.float32).reshape(-1))


# ------------------------------------------------------------------------------------------ graphs
def from_rows(n, rows, cols=None):
    """CSR with the given column list per row, in the given order; values 1, 2, 3, ... by position"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.asarray([c for r in rows for c in r], np.int32).reshape(-1)
    va = np.arange(1, ci.size + 1, dtype=np.float32)
    return (n, rp, ci, va) if cols is None else (n, cols, rp, ci, va)


def complete(n):
    return from_rows(n, [list(range(n)) for _ in range(n)])


def star(leaves):
    """vertex 0 adjacent to 1 .. leaves; every diagonal stored"""
    return from_rows(leaves + 1, [list(range(leaves + 1))] + [[0, i] for i in range(1, leaves + 1)])


def path(n):
    return from_rows(n, [[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)])


def upper_bidiagonal(n):
    """only (i, i + 1) stored: every edge is visible from one of its ends through A^T alone"""
    return from_rows(n, [[i + 1] if i + 1 < n else [] for i in range(n)])


def diagonal_only(n):
    return from_rows(n, [[i] for i in range(n)])


def messy():
    """empty rows, repeated entries, stored diagonals, unsorted rows, one-sided entries"""
    rows = [[], [1, 1, 3, 1], [0, 5, 0], [3], [], [6, 2, 6, 5, 5], [0], [7, 1, 7], [2, 4, 4], []]
    return from_rows(len(rows), rows)


def with_row_lengths(lengths, cols, seed=0, repeats=False):
    """a rows x cols matrix whose row i has lengths[i] entries in random order; with `repeats` columns are drawn with
    replacement from a quarter of the range, so most rows store a column several times"""
    rng = np.random.default_rng(seed)
    rows = []
    for length in lengths:
        if repeats:
            rows.append(list(rng.integers(0, max(cols // 4, 1), length)))
        else:
            rows.append(list(rng.permutation(cols)[:length]) if length <= cols else
                        list(rng.integers(0, cols, length)))
    n, c, rp, ci, va = from_rows(len(lengths), rows, cols)
    va = rng.uniform(-1.0, 1.0, ci.size).astype(np.float32)
    return n, c, rp, ci, va


def tridiagonal(n):
    """path(n) built without a Python loop, for the sizes past a grid cap"""
    i = np.arange(n, dtype=np.int64)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return n, rp, cols[order].astype(np.int32), np.ones(order.size, np.float32)


def coalesced(n, rp, ci, va):
    """the same matrix with every row's columns ascending and the stored entries of one position added up (fp32, in
    storage order): the form ilu0_csr and ic0_csr ask for.  The graph, and so the colouring, is unchanged."""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    keys, where = np.unique(rows * n + np.asarray(ci, np.int64), return_inverse=True)
    sums = np.zeros(keys.size, np.float32)
    for j in range(len(where)):                          # np.add.at's order is unspecified; this one is storage order
        sums[where[j]] = np.float32(sums[where[j]] + va[j])
    new_rp = np.concatenate([[0], np.cumsum(np.bincount(keys // n, minlength=n))]).astype(np.int32)
    return n, new_rp, (keys % n).astype(np.int32), sums


LIBRARY = {
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
    "random_spd(500, 7, 3)": lambda: spd.random_spd(500, 7, 3),
    "convdiff2d(16)": lambda: nonsym.convdiff2d(16),
}

# the colour counts at seed 0 that tests/golden/reorder_restate.json records
COUNTED = {
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
    "random_spd(500, 7, 3)": lambda: spd.random_spd(500, 7, 3),
    "poisson2d(64)": lambda: spd.poisson2d(64),
    "poisson3d(16)": lambda: spd.poisson3d(16),
    "random_spd(1025, 7, 5)": lambda: spd.random_spd(1025, 7, 5),
}
QUOTED_COLORS = {"poisson2d(24)": 4, "poisson3d(8)": 5, "random_spd(500, 7, 3)": 9, "poisson2d(64)": 5,
                 "poisson3d(16)": 6, "random_spd(1025, 7, 5)": 9}

SMALL = {
    "single": lambda: from_rows(1, [[0]]),
    "edge": lambda: from_rows(2, [[1], [0]]),
    "diagonal_only": lambda: diagonal_only(7),
    "messy": messy,
    "K5": lambda: complete(5),
    "path(10)": lambda: path(10),
    "star(9)": lambda: star(9),
    "upper_bidiagonal(9)": lambda: upper_bidiagonal(9),
}
