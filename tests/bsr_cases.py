"""Block CSR test data and the four definitions of include/spmv/bsr.h restated in numpy: CSR -> BSR, BSR -> CSR with
both flags, the ordered product in float32 with separate roundings, and an int64 exact reference.  A plain module,
imported by tests/test_bsr_host.py (which proves every claim made here on the CPU) and tests/test_gpu_bsr.py."""
import numpy as np

import exact_data as ed

BLOCK_DIMS = (2, 3, 4, 8)
LANES = ed.LANES
NAN_PAYLOAD = np.uint32(0x7FC12345)
DENORMAL = np.uint32(0x00000007)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """Three arrays each: ints equal, values equal bit for bit."""
    for k in range(2):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, "ints", k)
    assert got[2].size == want[2].size and np.array_equal(bits(got[2]), bits(want[2])), (what, "value bits")


def blocks_along(n, b):
    return -(-n // b)


# ------------------------------------------------------------------------------------------ the definitions
def from_csr(m, n, b, rp, ci, va):
    """(block_row_ptrs, block_cols, values flat) of bsr_from_csr_cpu's rule; rows strictly ascending."""
    rp, ci, va = np.asarray(rp, np.int64), np.asarray(ci, np.int64), np.asarray(va, np.float32)
    nbr, nbc = blocks_along(m, b), blocks_along(n, b)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    key = (row // b) * max(nbc, 1) + ci // b
    uniq = np.unique(key)
    at = np.searchsorted(uniq, key)
    values = np.zeros(uniq.size * b * b, np.float32)
    values[(at * b + row % b) * b + ci % b] = va
    brp = np.concatenate([[0], np.cumsum(np.bincount(uniq // max(nbc, 1), minlength=nbr))]).astype(np.int32)
    return brp, (uniq % max(nbc, 1)).astype(np.int32), values


def to_csr(m, n, b, brp, bc, bv, keep_zeros):
    """(row_ptrs, cols, values) of bsr_to_csr_cpu's rule: sorted rows; every position inside the matrix, or the ones
    whose value is not +-0.0f."""
    brp, bc = np.asarray(brp, np.int64), np.asarray(bc, np.int64)
    bv = np.asarray(bv, np.float32).reshape(-1, b, b)
    I = np.repeat(np.arange(brp.size - 1, dtype=np.int64), np.diff(brp))
    rows = (I[:, None, None] * b + np.arange(b)[None, :, None]) + np.zeros((1, 1, b), np.int64)
    cols = (bc[:, None, None] * b + np.arange(b)[None, None, :]) + np.zeros((1, b, 1), np.int64)
    keep = (rows < m) & (cols < n)
    if not keep_zeros:
        keep &= (bv.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0
    rows, cols, vals = rows[keep], cols[keep], bv[keep]
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return rp, cols[order].astype(np.int32), vals[order]


def ordered_csr_product(rp, ci, va, x):
    """s = +0; s = fl(s + fl(v * x)) over each row's entries in stored order, in float32 (spmv_cpu_csr's sum)."""
    rp = np.asarray(rp, np.int64)
    va, x = np.asarray(va, np.float32), np.asarray(x, np.float32)
    lens = np.diff(rp)
    y = np.zeros(lens.size, np.float32)
    with np.errstate(all="ignore"):
        for k in range(int(lens.max()) if lens.size else 0):
            live = np.flatnonzero(lens > k)
            p = rp[live] + k
            y[live] = y[live] + va[p] * x[ci[p]]
    return y


def ordered_product(m, n, b, brp, bc, bv, x):
    """spmv_cpu_bsr's sum: the blocks of the block row in stored order, the positions inside the matrix only."""
    return ordered_csr_product(*to_csr(m, n, b, brp, bc, bv, 1), x)


def exact_product(m, n, b, brp, bc, bv, x):
    """y in int64 arithmetic as float32, after check_exact's condition was asserted: every order gives these bits."""
    rp, ci, va = to_csr(m, n, b, brp, bc, bv, 1)
    ed.check_exact(rp, ci, va, np.asarray(x, np.float32))
    return ed.exact_reference(rp, ci, va, x)


# ------------------------------------------------------------------------------------------ CSR generators
def csr_from_rows(rows):
    """rows: a list of lists of (column, value), columns ascending."""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float32)
    return rp, ci, va


def random_csr(rng, m, n, density, wide=False):
    """Sorted rows without repeats.  wide: values with exponents over +-20 decades, both signs."""
    mask = rng.random((m, n)) < density if m * n else np.zeros((m, n), bool)
    rows, cols = np.nonzero(mask)
    if wide:
        vals = (rng.uniform(1, 10, rows.size) * 10.0 ** rng.integers(-20, 21, rows.size) * rng.choice([-1, 1], rows.size))
    else:
        vals = rng.uniform(-4, 4, rows.size)
    vals = vals.astype(np.float32)
    vals[vals == 0] = 1.0
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    return rp, cols.astype(np.int32), vals


def wide_x(rng, n):
    """Finite x with exponents over +-20 decades, both signs, a tenth zeros and a tenth -0.0 (the first element is
    +0.0, the last -0.0)."""
    x = (rng.uniform(1, 10, n) * 10.0 ** rng.integers(-20, 21, n) * rng.choice([-1, 1], n)).astype(np.float32)
    x[rng.random(n) < 0.1] = 0.0
    x[rng.random(n) < 0.1] = -0.0
    x[0], x[-1] = 0.0, -0.0
    assert np.isfinite(x).all()
    return x


def with_specials(rng, arrays):
    """-0.0f, a NaN with a payload, a denormal and an explicit zero written over four entries (needs nnz >= 4)."""
    rp, ci, va = arrays
    va = va.copy()
    at = rng.choice(va.size, size=4, replace=False)
    va.view(np.uint32)[at] = [0x80000000, NAN_PAYLOAD, DENORMAL, 0]
    return rp, ci, va


def structured(b, rng):
    """Block rows: two empty at the start; one whose b rows touch pairwise disjoint block columns; one empty; one whose
    rows all touch the same two block columns; one whose only entry sits in its last row, in the matrix's last column;
    one full block row; two empty at the end.  n = 9 b."""
    n = 9 * b
    val = lambda: float(np.float32(rng.uniform(-3, 3))) or 1.0
    rows = [[] for _ in range(2 * b)]
    rows += [[(r * b + (r * 3) % b, val())] for r in range(b)]
    rows += [[] for _ in range(b)]
    rows += [[(1 * b + (r % b), val()), (4 * b, val()), (4 * b + b - 1, val())] for r in range(b)]
    rows += [[] for _ in range(b - 1)] + [[(n - 1, val())]]
    rows += [[(c, val()) for c in range(n)] for _ in range(b)]
    rows += [[] for _ in range(2 * b)]
    return len(rows), n, csr_from_rows(rows)


def long_block_row(b, rng, blocks=4097):
    """One block row of `blocks` blocks (past a scan tile): block J is touched by row J % b alone, every 5th also by
    the last row."""
    n = blocks * b - 1
    rows = [[] for _ in range(b)]
    for J in range(blocks):
        rows[J % b].append((min(J * b + (J * 7) % b, n - 1), float(rng.integers(1, 9))))
        if J % 5 == 0 and J % b != b - 1:
            rows[b - 1].append((J * b, float(-rng.integers(1, 9))))
    return b, n, csr_from_rows(rows)


def many_block_rows(b, rng, block_rows, cols_blocks=37):
    """block_rows block rows of one or two blocks each, one entry per scalar row (rows spread over the two blocks), the
    last block row cut short: m = block_rows * b - 1.  Every 13th block row is empty."""
    m, n = block_rows * b - 1, cols_blocks * b - 1
    i = np.arange(m, dtype=np.int64)
    I = i // b
    first = (I * 5) % cols_blocks
    second = (first + 1 + (I % 3)) % cols_blocks
    two = (I % 2 == 1) & (i % b >= b // 2)
    J = np.where(two, second, first)
    cols = np.minimum(J * b + (i % b + I) % b, n - 1)
    live = I % 13 != 12
    rp = np.concatenate([[0], np.cumsum(live)]).astype(np.int32)
    vals = (rng.integers(1, 9, size=m) * rng.choice([-1, 1], size=m)).astype(np.float32)
    return m, n, (rp, cols[live].astype(np.int32), vals[live])


def conversion_cases(b):
    """[(name, m, n, (rp, ci, va))]: every shape the conversion tests run, host and device."""
    rng = np.random.default_rng(100 + b)
    out = []
    for name, m, n, density in (("1x1", 1, 1, 1.0), ("bxb", b, b, 0.6), ("(b+1)x(2b-1)", b + 1, 2 * b - 1, 0.5),
                                ("rows no multiple", 5 * b + 1, 6 * b, 0.2), ("cols no multiple", 4 * b, 5 * b + b - 1, 0.2),
                                ("neither a multiple", 7 * b - 1, 9 * b + 1, 0.15), ("dense", 3 * b + 1, 2 * b + 1, 1.0),
                                ("nnz = 0", 3 * b, 4 * b, 0.0), ("m = 0", 0, 5, 0.0), ("n = 0", 5, 0, 0.0),
                                ("ragged", 211, 97, 0.06)):
        out.append((name, m, n, random_csr(rng, m, n, density)))
    out.append(("structured",) + structured(b, rng))
    out.append(("long block row",) + long_block_row(b, rng))
    out.append(("4097 block rows",) + many_block_rows(b, rng, 4097))
    m, n = 9 * b + 2, 8 * b + 1
    out.append(("specials", m, n, with_specials(rng, random_csr(rng, m, n, 0.3))))
    return out


# ------------------------------------------------------------------------------------------ exact BSR matrices
def exact_bsr(rng, b, m, n, block_lens):
    """(brp, bc, bv, x): the given blocks per block row at distinct ascending block columns, every position of every
    block a non-zero integer in [-8, 8] (positions outside the matrix +0.0f), x non-zero integers in [-64, 64]."""
    nbr, nbc = blocks_along(m, b), blocks_along(n, b)
    block_lens = np.asarray(block_lens, np.int64)
    assert block_lens.size == nbr and int(block_lens.max(initial=0)) <= nbc
    brp = np.concatenate([[0], np.cumsum(block_lens)]).astype(np.int32)
    bc = np.empty(int(brp[-1]), np.int32)
    short = block_lens <= 2
    start = rng.integers(0, max(nbc - 2, 1), size=nbr)
    for k in range(2):                                                        # rows of one or two blocks, vectorised
        rows = np.flatnonzero(short & (block_lens > k))
        bc[brp[rows] + k] = np.minimum(start[rows] + k * (1 + rows % 2), nbc - 1) if nbc > 1 else 0
    for I in np.flatnonzero(~short):
        bc[brp[I]:brp[I + 1]] = np.sort(rng.choice(nbc, size=int(block_lens[I]), replace=False))
    if nbc == 1:
        assert int(block_lens.max(initial=0)) <= 1
    bv = (rng.integers(1, 9, size=(bc.size, b, b)) * rng.choice([-1, 1], size=(bc.size, b, b))).astype(np.float32)
    I = np.repeat(np.arange(nbr, dtype=np.int64), block_lens)
    outside = ((I[:, None, None] * b + np.arange(b)[None, :, None]) >= m) | \
              ((bc.astype(np.int64)[:, None, None] * b + np.arange(b)[None, None, :]) >= n)
    bv[outside] = 0.0
    x = ed.nonzero_x(rng, n)
    return brp, bc, bv.reshape(-1), x


def sweep_lens(L):
    """Block-row lengths of the lane sweep: 0, 1, L - 1, L, L + 1, 4 L + 1 and one of about 1000 blocks, twice over
    with short rows between, so that the long ones meet every slot of a wavefront."""
    edge = [0, 1, max(L - 1, 0), L, L + 1, 4 * L + 1, 1003]
    return edge + [2, 0, 3] + edge[::-1] + [1]


def sweep_case(L, b):
    """(m, n, brp, bc, bv, x) of the small lane-sweep matrix for lane count L and block size b; neither dimension is
    a multiple of b."""
    lens = sweep_lens(L)
    rng = np.random.default_rng(1000 * L + b)
    m, n = len(lens) * b - 1, 1100 * b - (b - 1)
    return (m, n) + exact_bsr(rng, b, m, n, lens)


def capped_case(L, b):
    """(m, n, brp, bc, bv, x): exact_data.LANE_SIZES[L] block rows, past one trip of the grid at L lanes, one or two
    blocks each (every 7th empty)."""
    nbr = ed.LANE_SIZES[L]
    rng = np.random.default_rng(5000 + 10 * L + b)
    lens = 1 + (np.arange(nbr) % 2)
    lens[::7] = 0
    m, n = nbr * b - 1, 41 * b - 1
    return (m, n) + exact_bsr(rng, b, m, n, lens)


def forced(monkeypatch, lanes):
    if lanes:
        monkeypatch.setenv("SPMV_DEBUG", "bsr_lanes=%d" % lanes)
    else:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
