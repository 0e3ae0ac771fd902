"""Structure families and numpy restatements shared by tests/test_sptrsv_analysis_host.py and
tests/test_gpu_sptrsv_analysis.py (the device-side level analysis).  Every family is
(n, row_ptrs, col_indices, values) with int32 structure arrays.  A plain module, not a conftest."""
import numpy as np

NARROW = 256             # csrc/internal.h kSptrsvNarrowRows
MAX_RUN_LEVELS = 8192    # csrc/internal.h kSptrsvMaxRunLevels
BLOCK = 256              # csrc/device_common.h kBlock
MAX_GRID = 256 * 8       # csrc/device_common.h kMaxResidentBlocks: capped_grid's reach


def from_coo(n, rows, cols, keep_order=False):
    """CSR of the entries in the order given inside each row (keep_order) or sorted by column, duplicates kept"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.argsort(rows, kind="stable") if keep_order else np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    ci = cols[order].astype(np.int32)
    return n, rp, ci, (1.0 + 0.25 * (np.arange(ci.size) % 7)).astype(np.float32)


def diagonal(n, with_diagonal=True):
    idx = np.arange(n if with_diagonal else 0)
    return from_coo(n, idx, idx)


def chain(n):
    """(i, i-1), (i, i), (i, i+1): each triangle is bidiagonal, one row per level"""
    i = np.arange(n)
    return from_coo(n, np.concatenate([i[1:], i, i[:-1]]), np.concatenate([i[1:] - 1, i, i[:-1] + 1]))


def staircase(widths):
    """LOWER levels of the given widths: row p of level l > 0 stores (i, one row of level l - 1) and its diagonal"""
    starts = np.concatenate([[0], np.cumsum(widths)])
    n = int(starts[-1])
    rows, cols = [np.arange(n)], [np.arange(n)]
    for l in range(1, len(widths)):
        mine = np.arange(starts[l], starts[l + 1])
        rows.append(mine)
        cols.append(starts[l - 1] + (mine - starts[l]) % widths[l - 1])
    return from_coo(n, np.concatenate(rows), np.concatenate(cols))


def flipped(case):
    """P A P with P: i -> n - 1 - i: the LOWER triangle becomes the UPPER one"""
    n, rp, ci, _ = case
    r = np.repeat(np.arange(n), np.diff(rp))
    return from_coo(n, n - 1 - r, n - 1 - ci.astype(np.int64))


def arrow(n):
    """diagonal, a dense last row and a dense first column: a long row and a hub column"""
    i = np.arange(n)
    rows = np.concatenate([i, np.full(n - 1, n - 1), i[1:-1]])
    cols = np.concatenate([i, i[:-1], np.zeros(n - 2, np.int64)])
    return from_coo(n, rows, cols)


def hub_in_a_wide_level(n=4000, first=300):
    """LOWER: a level 0 of `first` rows (wider than NARROW) whose row 0 has n - first dependents (more than the 2048
    past which a column is walked by a whole wavefront); every other row stores (i, 0), (i, 1 + i % (first - 1)), (i, i)"""
    i = np.arange(n)
    rest = i[first:]
    rows = np.concatenate([i, rest, rest])
    cols = np.concatenate([i, np.zeros(rest.size, np.int64), 1 + rest % (first - 1)])
    return from_coo(n, rows, cols)


def strictly_lower(n, per_row=3, seed=5):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(1, n), per_row)
    cols = (rng.random(rows.size) * rows).astype(np.int64)       # 0 <= c < row
    pairs = np.unique(rows * n + cols)
    return from_coo(n, pairs // n, pairs % n)


def messy(nonsym, n=2000, seed=9):
    """random_nonsym's pattern with unsorted columns, duplicated entries, missing diagonals, empty rows and rows whose
    entries all lie on one side of the diagonal"""
    rng = np.random.default_rng(seed)
    _, rp, ci, _ = nonsym.random_nonsym(n, 7, seed)
    r = np.repeat(np.arange(n), np.diff(rp))
    c = ci.astype(np.int64)
    keep = np.ones(r.size, bool)
    keep &= ~((r == c) & (r % 11 == 3))                          # missing diagonals
    keep &= r % 17 != 5                                          # empty rows
    keep &= ~((r % 13 == 7) & (c < r))                           # upper side (and diagonal) only
    keep &= ~((r % 13 == 8) & (c > r))                           # lower side (and diagonal) only
    r, c = r[keep], c[keep]
    again = rng.random(r.size) < 0.2                             # duplicates, the diagonal's among them
    r, c = np.concatenate([r, r[again]]), np.concatenate([c, c[again]])
    shuffle = rng.permutation(r.size)                            # unsorted inside the rows
    return from_coo(n, r[shuffle], c[shuffle], keep_order=True)


def families(spd, nonsym):
    """the structure families of tests/test_gpu_sptrsv_analysis.py: name -> (n, rp, ci, va)"""
    stairs = staircase([255, 256, 257, 1, 600, 256])
    return {
        "n=1": diagonal(1),
        "n=1 without its diagonal": diagonal(1, with_diagonal=False),
        "n=2": chain(2),
        "diagonal(255)": diagonal(255),
        "diagonal(256)": diagonal(256),
        "diagonal(257)": diagonal(257),
        # one row per thread at the grid cap is MAX_GRID * BLOCK rows: a second trip of the grid-stride loops
        "diagonal past the grid": diagonal(MAX_GRID * BLOCK + 7),
        "chain(300)": chain(300),
        "chain past the run limit": chain(MAX_RUN_LEVELS + 5),
        "staircase": stairs,
        "staircase flipped": flipped(stairs),
        "poisson2d(64)": spd.poisson2d(64),
        "poisson3d(16)": spd.poisson3d(16),
        "poisson3d(32)": spd.poisson3d(32),
        "messy(2000)": messy(nonsym, 2000),
        "arrow(5000)": arrow(5000),
        "strictly lower(3000)": strictly_lower(3000),
        "hub in a wide level": hub_in_a_wide_level(),
        "hub in a wide level flipped": flipped(hub_in_a_wide_level()),
    }


FAMILY_NAMES = ("n=1", "n=1 without its diagonal", "n=2", "diagonal(255)", "diagonal(256)", "diagonal(257)",
                "diagonal past the grid", "chain(300)", "chain past the run limit", "staircase", "staircase flipped",
                "poisson2d(64)", "poisson3d(16)", "poisson3d(32)", "messy(2000)", "arrow(5000)",
                "strictly lower(3000)", "hub in a wide level", "hub in a wide level flipped")


def one_sided_variants(spd):
    """sorted rows, every diagonal stored: name -> (case, pattern is structurally symmetric)"""
    n, rp, ci, va = spd.poisson2d(12)
    r = np.repeat(np.arange(n), np.diff(rp))
    drop_upper = ~((r == 40) & (ci == 41))                       # (41, 40) stays: row 41 is one-sided
    drop_lower = ~((r == 77) & (ci == 76))                       # (76, 77) stays: row 76 is one-sided
    return {
        "poisson2d(12)": ((n, rp, ci, va), True),
        "poisson3d(6)": (spd.poisson3d(6), True),
        "chain(40)": (chain(40), True),
        "arrow(50)": (from_coo(50, *_symmetrised(arrow(50))), True),
        "arrow(50) one-sided": (arrow(50), False),
        "staircase": (staircase([3, 4, 5, 1, 6]), False),
        "lower bidiagonal": (from_coo(30, np.concatenate([np.arange(30), np.arange(1, 30)]),
                                      np.concatenate([np.arange(30), np.arange(29)])), False),
        "poisson2d(12) less (40,41)": (from_coo(n, r[drop_upper], ci[drop_upper]), False),
        "poisson2d(12) less (77,76)": (from_coo(n, r[drop_lower], ci[drop_lower]), False),
        "diagonal(9)": (diagonal(9), True),
    }


def _symmetrised(case):
    n, rp, ci, _ = case
    r = np.repeat(np.arange(n), np.diff(rp))
    pairs = np.unique(np.concatenate([r * n + ci, ci.astype(np.int64) * n + r]))
    return pairs // n, pairs % n


# ---- numpy restatements --------------------------------------------------------------------------------------
def one_sided_row(n, rp, ci):
    """the device rule: the lowest row i that stores an (i, k), k != i, whose (k, i) is not stored; -1 when none"""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    c = ci.astype(np.int64)
    off = r != c
    lonely = off & ~np.isin(c * n + r, r * n + c)
    return int(r[lonely].min()) if lonely.any() else -1


def first_unsorted_row(n, rp, ci):
    r = np.repeat(np.arange(n), np.diff(rp))
    bad = np.zeros(ci.size, bool)
    if ci.size > 1:
        bad[1:] = (r[1:] == r[:-1]) & (ci[1:] <= ci[:-1])
    return int(r[bad].min()) if bad.any() else -1


def triangle_nnz(n, rp, ci, uplo):
    r = np.repeat(np.arange(n), np.diff(rp))
    return int(((ci >= r) if uplo else (ci <= r)).sum())


def launches(level_ptr):
    """group_levels of sptrsv_host.cpp: a level wider than NARROW alone, consecutive narrower ones together, at most
    MAX_RUN_LEVELS of them"""
    count, run = 0, 0            # run: levels in the open run of narrow levels, 0 = none open
    for rows in np.diff(level_ptr):
        if rows <= NARROW and 0 < run < MAX_RUN_LEVELS:
            run += 1
        else:
            count += 1
            run = 1 if rows <= NARROW else 0
    return count
