"""Shared helpers of tests/test_csr_ops_host.py and tests/test_gpu_csr_ops.py: CSR builders with strictly ascending
rows, the plain restatement of the sum's three-case rule (include/spmv/csr_ops.h) in np.float32 arithmetic, and the
row-shape generator of the lane sweep.  A plain module, not a conftest."""
import numpy as np

from spgemm_cases import assert_same, bits, csr_from_rows, random_csr        # noqa: F401  (the tests use them from here)

LANES = (1, 2, 4, 8, 16, 32, 64)
OVERLAPS = ("interleaved", "identical", "a_left_of_b", "b_left_of_a", "first_common", "last_common", "every_second")
LONG_TILES = 32          # kLongTiles (csrc/csr_ops.hip): a row of more than LONG_TILES * L entries in A and B together
                         # is walked by its whole wavefront instead of its group of L lanes (L < 64)
SPECIALS = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-40, 3e38, -3e38], np.float32)


def empty(rows):
    return np.zeros(rows + 1, np.int32), np.empty(0, np.int32), np.empty(0, np.float32)


def with_specials(rng, arrays, share=0.1):
    """The same matrix with a share of its values replaced by zeros, infinities, NaN, denormals and huge values."""
    rp, ci, va = arrays
    va = va.copy()
    hit = rng.random(va.size) < share
    va[hit] = rng.choice(SPECIALS, size=int(hit.sum()))
    return rp, ci, va


def integer_csr(rng, rows, cols, density, vmax=8):
    """Strictly ascending rows with non-zero integer values in [-vmax, vmax]."""
    rp, ci, va = random_csr(rng, rows, cols, density)
    va = (rng.integers(1, vmax + 1, size=va.size) * rng.choice([-1, 1], size=va.size)).astype(np.float32)
    return rp, ci, va


def add_loop(m, alpha, a, beta, b):
    """The definition, restated: per row the two-pointer merge; fl(alpha a), fl(beta b) or fl(fl(alpha a) + fl(beta b))."""
    arp, aci, ava = a
    brp, bci, bva = b
    alpha, beta = np.float32(alpha), np.float32(beta)
    rp = np.zeros(m + 1, np.int32)
    ci, va = [], []
    with np.errstate(all="ignore"):
        for i in range(m):
            p, q = int(arp[i]), int(brp[i])
            while p < arp[i + 1] or q < brp[i + 1]:
                ca = int(aci[p]) if p < arp[i + 1] else None
                cb = int(bci[q]) if q < brp[i + 1] else None
                if cb is None or (ca is not None and ca < cb):
                    ci.append(ca)
                    va.append(np.float32(alpha * np.float32(ava[p])))
                    p += 1
                elif ca is None or cb < ca:
                    ci.append(cb)
                    va.append(np.float32(beta * np.float32(bva[q])))
                    q += 1
                else:
                    left = np.float32(alpha * np.float32(ava[p]))
                    right = np.float32(beta * np.float32(bva[q]))
                    ci.append(ca)
                    va.append(np.float32(left + right))
                    p += 1
                    q += 1
            rp[i + 1] = len(ci)
    return rp, np.asarray(ci, np.int32), np.asarray(va, np.float32)


def common_per_row(a, b):
    """Columns stored in both matrices, per row."""
    return np.asarray([np.intersect1d(a[1][a[0][i]:a[0][i + 1]], b[1][b[0][i]:b[0][i + 1]]).size
                       for i in range(a[0].size - 1)], np.int64)


def host_sum(spmv, m, n, alpha, a, beta, b):
    """csr_add_cpu of freshly built host matrices: (status, (row_ptrs, cols, vals))."""
    A = spmv.csr_from_arrays(m, n, *a)
    B = spmv.csr_from_arrays(m, n, *b)
    C = spmv.csr_create(0, 0, 0)
    status = spmv.csr_add_cpu(C, alpha, A, beta, B)
    got = spmv.csr_host_arrays(C) if status == 0 else None
    shape = (C.contents.num_rows, C.contents.num_cols, C.contents.nnz)
    for M in (A, B, C):
        spmv.csr_destroy(M)
    if status == 0:
        assert shape == (m, n, got[1].size)
    return status, got


# ---- the row shapes of the lane sweep ----------------------------------------------------------------------------
def overlap_positions(form, la, lb):
    """Abstract ascending positions of the two rows for one overlap form, or None where the form needs an entry a row
    does not have."""
    a, b = np.arange(la, dtype=np.int64), np.arange(lb, dtype=np.int64)
    if form == "interleaved":
        return 2 * a, 2 * b + 1
    if form == "identical":                       # the shorter row is a prefix of the longer one
        return a, b
    if form == "a_left_of_b":
        return a, la + b
    if form == "b_left_of_a":
        return lb + a, b
    if form == "first_common":
        if la == 0 or lb == 0:
            return None
        return np.concatenate([[0], 2 * a[1:]]), np.concatenate([[0], 2 * b[1:] + 1])
    if form == "last_common":
        if la == 0 or lb == 0:
            return None
        top = 2 * max(la, lb) + 2
        return np.concatenate([2 * a[:-1], [top]]), np.concatenate([2 * b[:-1] + 1, [top]])
    if form == "every_second":                    # A's entries 0, 2, 4, ... are B's too, as far as B reaches; the
        shared = 3 * a[::2][:lb]                  # rest of B lies between A's entries
        own = 3 * np.arange(lb - shared.size, dtype=np.int64) + 1
        return 3 * a, np.sort(np.concatenate([shared, own]))
    raise ValueError(form)


def lane_rows(L, n, seed):
    """The matrix pair of the lane sweep: one row per (len(A), len(B), overlap form), lengths from
    {0, 1, L-1, L, L+1, 2L+1}.  Every non-empty union starts at column 0 and, with two or more columns, ends at
    n - 1; the columns between are drawn from [1, n - 1)."""
    rng = np.random.default_rng(seed)
    lengths = sorted({0, 1, max(L - 1, 0), L, L + 1, 2 * L + 1})
    a_rows, b_rows = [], []
    for la in lengths:
        for lb in lengths:
            for form in OVERLAPS:
                pos = overlap_positions(form, la, lb)
                if pos is None:
                    continue
                union, inverse = np.unique(np.concatenate(pos), return_inverse=True)
                cols = np.empty(union.size, np.int64)
                if union.size:
                    cols[0] = 0
                if union.size > 1:
                    cols[-1] = n - 1
                    cols[1:-1] = np.sort(rng.choice(n - 2, size=union.size - 2, replace=False)) + 1
                ca, cb = cols[inverse[:la]], cols[inverse[la:]]
                assert np.all(np.diff(ca) > 0) and np.all(np.diff(cb) > 0)
                a_rows.append(list(zip(ca.tolist(), rng.uniform(-3, 3, la).astype(np.float32).tolist())))
                b_rows.append(list(zip(cb.tolist(), rng.uniform(-3, 3, lb).astype(np.float32).tolist())))
    return csr_from_rows(a_rows), csr_from_rows(b_rows)


def short_rows(rng, m, n=64):
    """m rows of one to three entries each, strictly ascending columns below n (>= 61), built without a Python loop."""
    assert n >= 61
    steps = rng.integers(1, 21, size=(m, 3))
    steps[:, 0] -= 1
    cols = np.cumsum(steps, axis=1)
    lens = rng.integers(1, 4, size=m)
    keep = np.arange(3)[None, :] < lens[:, None]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = cols[keep].astype(np.int32)
    return rp, ci, rng.uniform(-2, 2, size=ci.size).astype(np.float32)
