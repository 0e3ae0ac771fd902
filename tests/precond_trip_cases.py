"""Data of the preconditioner kernels' second grid-stride trips (tests/test_precond_trips_host.py proves every claim
made here on the CPU, tests/test_gpu_precond_trips.py runs the shapes on the device).  A plain module, like
exact_data.py: vectorised numpy throughout, because the largest case has about 525 k rows.

The row kernels take row_trip(L) rows a trip (exact_data.py), the element-wise kernels VEC_TRIP elements.  A row case
is exact_data.LANE_SIZES' rule, row_trip(L) + 256 / L + 1: its second trip starts with one full workgroup and one
workgroup of a single row.  An element-wise case has VEC_TRIP + 257 elements.

1. IC(0) / ILU(0)   block-diagonal matrices of 3 x 3 pieces, rows interleaved by a fixed permutation that keeps each
                    piece's order: three LOWER levels, each `blocks` rows wide.  The exact tier takes its pieces from
                    the rule of ic0_cases.exact_tridiagonal / ilu0_cases.exact_tridiagonal; prove_chain_exact is the
                    fixed-point prover of those files for matrices whose rows and columns hold at most one entry left
                    of (below) the diagonal, one level at a time.
2. sptrsv_csr_multi exact_data.two_level_triangle with k integer columns, B = T X in integers.
3. FSAI             band matrices whose half-bandwidth changes at row 2048 G (G = FSAI_ROWS_PER_BLOCK rows a
                    workgroup and trip), so the second trip meets other row lengths than the first; the exact tier
                    past the cap; the structure kernels' rejected inputs.
                    The exact tier proves ONE PERIOD of 24 rows with fsai_cases.prove_exact and repeats it 342 times:
                    fsai_cases.exact_blocks builds the dense n x n factor and its product, which at n = 8208 is half
                    a gigabyte and an integer matrix product of 5e11 operations.
                    A row of a lower pattern holds at most i + 1 entries, so the first trip of workgroup 0 (rows
                    0 .. G - 1) holds rows of 1 .. G entries whatever the bandwidth, and with n = 2048 G + G + 1 the
                    second trip's two workgroups held only those and rows G .. 2 G - 1 before.  The "deep" cases
                    (64 more rows; an addition to the issue's two per pair) let the second trip reach workgroups
                    whose first-trip rows all had the class's full length.
4. AMG V-cycle      tridiag(-1, 2, -1) with pair aggregates, two levels, a Jacobi-solved coarsest level.  FastProver is
                    the vectorised twin of amg_cases.Prover in int64 fixed point; JacobiProver adds the Jacobi
                    coarsest level to the Fraction prover, and the host test holds the twin to it.
5. AMG setup        the shapes that put the MIS-2 grid at its cap and the element-wise kernels past theirs.
6. Smoothed AMG     the same family with omega_p = 1: P averages (1/2, 1/2), the Galerkin matrix has 1/2 on its whole
                    diagonal, -1/4 at distance two and a stored 0 at distance one, wd is 1/4 and 1, and the weighted
                    cycle is dyadic throughout.  SmoothedProver is FastProver on the CSR arrays of the levels, of P
                    and of PT as read from the host twins (no closed form); SmoothedFractions is its Fraction twin.
                    PT has half of A's rows, so the three row sweeps pass their caps at different n.

Nothing here had to be changed to be admitted: every V-cycle case of the issues is exact as stated (the host tests
print the widths)."""
from fractions import Fraction

import numpy as np

import amg_cases as ac
import amg_smoothed_cases as sc
import exact_data as ed
import fsai_cases as fc
from exact_data import EXACT_LIMIT, ROW_TRIP_THREADS, VEC_TRIP, row_trip
from ilu0_cases import csr_from_coo, rows_of

BLOCK = ROW_TRIP_THREADS // 2048              # threads of a workgroup (kBlock)
ROW_BLOCKS = ROW_TRIP_THREADS // BLOCK        # kMaxResidentBlocks: workgroups of a row kernel's largest grid
VEC_BLOCKS = VEC_TRIP // BLOCK                # kVecBlocks
TRIP_LANES = (64, 8)                          # forced lane counts of the row kernels (exact_data.SPTRSV_TRIP_LANES' precedent)
VEC_ROWS = VEC_TRIP + 257                     # an element-wise case


def past_row_cap(L, rows_per_block=None):
    """row_trip(L) + 256 / L + 1 (exact_data.LANE_SIZES), or for another rows-per-workgroup count G: 2048 G + G + 1"""
    if rows_per_block is None:
        return ed.LANE_SIZES[L] if L > 1 else row_trip(1) + BLOCK + 1
    return ROW_BLOCKS * rows_per_block + rows_per_block + 1


def trips(items, per_trip):
    return -(-items // per_trip)


def row_grid(items, per_block):
    """capped_grid (csrc/device_common.h)"""
    return max(1, min(trips(items, per_block), ROW_BLOCKS))


def vec_grid(items):
    return max(1, min(trips(items, BLOCK), VEC_BLOCKS))


def tridiagonal(n):
    """amg_cases.tridiagonal, vectorised"""
    i = np.arange(n, dtype=np.int64)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.concatenate([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)])
    return csr_from_coo(n, rows, cols, vals.astype(np.float32))


def _assemble(n, rows, cols, *values):
    rows, cols = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return (n, rp, cols[order].astype(np.int32)) + tuple(np.concatenate(v).astype(np.float32)[order] for v in values)


# ------------------------------------------------------------------------------------------ 1. IC(0) and ILU(0)
FACTOR_KINDS = ("ic", "ilu")
PROOF_BLOCKS = 40                             # the size at which the Python-loop provers check prove_chain_exact


def factor_blocks(L):
    return past_row_cap(L)


def interleave(blocks, seed=17):
    """pos[b, j] = the row that row j of piece b becomes: a fixed permutation of the 3 * blocks rows, each piece's
    three positions sorted, so that a piece's rows keep their order (the factor is that of the piece) and are far
    apart (level order is not row order)"""
    return np.sort(np.random.default_rng(seed).permutation(3 * blocks).reshape(blocks, 3), axis=1)


def _pieces(blocks, entries, pos):
    """entries: ((i, j), values[, factor]) of the 3 x 3 piece, one value per piece"""
    rows = [pos[:, i] for (i, j), *_ in entries]
    cols = [pos[:, j] for (i, j), *_ in entries]
    return _assemble(3 * blocks, rows, cols, *[[e[k] for e in entries] for k in range(1, len(entries[0]))])


def exact_factor_blocks(kind, blocks, seed=0):
    """(n, rp, ci, va, fact): `blocks` pieces by the rule of ic0_cases.exact_tridiagonal(3) (A = L L^T, L lower
    bidiagonal, d in {1, 2, 4, 8}, |e| <= min(2, d)) or ilu0_cases.exact_tridiagonal(3, seed=...) (A = L U, unit L),
    interleaved; fact is the factor in A's pattern"""
    rng = np.random.default_rng(seed)
    pos = interleave(blocks)
    if kind == "ic":
        d = rng.choice([1, 2, 4, 8], (3, blocks))
        e = rng.choice([-2, -1, 1, 2], (3, blocks))
        e = np.sign(e) * np.minimum(np.abs(e), d)
        entries = [((0, 0), d[0] * d[0], d[0]), ((0, 1), e[1] * d[0], e[1]),
                   ((1, 0), e[1] * d[0], e[1]), ((1, 1), d[1] * d[1] + e[1] * e[1], d[1]), ((1, 2), e[2] * d[1], e[2]),
                   ((2, 1), e[2] * d[1], e[2]), ((2, 2), d[2] * d[2] + e[2] * e[2], d[2])]
    else:
        l = rng.choice([-3, -2, -1, 1, 2, 3], (3, blocks))
        d = rng.choice([2, 3, 4, 5, -4], (3, blocks))
        u = rng.choice([-3, -2, -1, 1, 2, 3], (3, blocks))
        entries = [((0, 0), d[0], d[0]), ((0, 1), u[0], u[0]),
                   ((1, 0), l[1] * d[0], l[1]), ((1, 1), d[1] + l[1] * u[0], d[1]), ((1, 2), u[1], u[1]),
                   ((2, 1), l[2] * d[1], l[2]), ((2, 2), d[2] + l[2] * u[1], d[2])]
    return _pieces(blocks, entries, pos)


def random_factor_blocks(kind, blocks, seed=5):
    """(n, rp, ci, va): the dense diagonally dominant 3 x 3 blocks of ic0_cases.spd_blocks / ilu0_cases.block3,
    interleaved"""
    m = np.random.default_rng(seed).uniform(-1.0, 1.0, (blocks, 3, 3))
    idx = np.arange(3)
    if kind == "ic":
        m = (m + m.transpose(0, 2, 1)) / 2
        m[:, idx, idx] = 0.0
    m[:, idx, idx] = np.abs(m).sum(axis=2) + 1.0
    pos = interleave(blocks)
    return _pieces(blocks, [((i, j), m[:, i, j]) for i in range(3) for j in range(3)], pos)


def _isqrt(w):
    root = np.rint(np.sqrt(w.astype(np.float64))).astype(np.int64)
    assert (root * root == w).all(), "a pivot is no perfect square"
    return root


def prove_chain_exact(kind, n, rp, ci, va):
    """ic0_cases.prove_exact / ilu0_cases.prove_exact (shift = 0) for an integer matrix whose pattern is structurally
    symmetric with at most one entry left of the diagonal in every row and at most one below it in every column
    (disjoint chains), a level at a time in int64.  Asserts that every quotient, update and square root is exact and
    below 2^24 and that L L^T (L U) == A.  Off the pattern there is nothing to check: row i holds l_ik and the
    diagonal only and no other row holds column k below the diagonal, so no product of two rows lands outside the
    pattern (IC); row k's one entry right of its diagonal is (k,i), the mirror of the one entry below (k,k) (ILU).
    Returns (factor in A's pattern, level of every row)."""
    rows = rows_of(n, rp)
    cols = np.asarray(ci, np.int64)
    a = np.rint(np.asarray(va, np.float64)).astype(np.int64)
    assert (a == np.asarray(va, np.float64)).all()
    key = rows * n + cols
    assert (np.diff(key) > 0).all()                                   # rows ascend strictly
    mirror = np.searchsorted(key, cols * n + rows)
    assert (mirror < key.size).all() and (key[np.minimum(mirror, key.size - 1)] == cols * n + rows).all()
    lower, diag = cols < rows, cols == rows
    assert (np.bincount(rows[diag], minlength=n) == 1).all()
    assert np.bincount(rows[lower], minlength=n).max() <= 1 and np.bincount(cols[lower], minlength=n).max() <= 1
    dpos = np.flatnonzero(diag)
    lpos = np.full(n, -1, np.int64)
    lpos[rows[lower]] = np.flatnonzero(lower)
    parent = np.full(n, -1, np.int64)
    parent[rows[lower]] = cols[lower]
    level = np.zeros(n, np.int64)
    while True:
        deeper = np.where(parent >= 0, level[np.maximum(parent, 0)] + 1, 0)
        if np.array_equal(deeper, level):
            break
        level = deeper
    w = a.copy()
    for lev in range(int(level.max()) + 1):
        i = np.flatnonzero(level == lev)
        if lev > 0:
            k, p = parent[i], lpos[i]
            num, den = w[p], w[dpos[k]]
            assert (den > 0).all() if kind == "ic" else (den != 0).all()
            assert (num % den == 0).all()
            q = num // den
            assert (np.abs(q) < EXACT_LIMIT).all()
            w[p] = q
            if kind == "ic":
                w[mirror[p]] = q                                       # the mirror store to (k,i)
                w[dpos[i]] -= q * q
                assert (q * w[dpos[k]] == a[p]).all()                  # (L L^T)_ik
            else:
                w[dpos[i]] -= q * w[mirror[p]]                         # u_ii = a_ii - l_ik u_ki
                assert (q * w[dpos[k]] == a[p]).all()                  # (L U)_ik
                assert (w[dpos[i]] + q * w[mirror[p]] == a[dpos[i]]).all()
            assert (np.abs(w[dpos[i]]) < EXACT_LIMIT).all()
        if kind == "ic":
            assert (w[dpos[i]] > 0).all()
            w[dpos[i]] = _isqrt(w[dpos[i]])
            below = np.where(lev > 0, w[np.maximum(lpos[i], 0)], 0)
            assert (w[dpos[i]] * w[dpos[i]] + below * below == a[dpos[i]]).all()       # (L L^T)_ii
    out = w.astype(np.float32)
    assert (out.astype(np.int64) == w).all()
    return out, level


PIVOT_ROWS = dict(negative=VEC_TRIP + 3, nan=VEC_TRIP + 100, zero=VEC_TRIP + 256)
PIVOT_BAD = dict(ic=PIVOT_ROWS["negative"], ilu=PIVOT_ROWS["nan"])     # ILU takes a negative pivot


def pivot_scan_matrix(clean=False):
    """diag(4) of VEC_ROWS rows; unless clean, one negative, one NaN and one zero diagonal, all in rows >= VEC_TRIP"""
    va = np.full(VEC_ROWS, 4.0, np.float32)
    if not clean:
        va[PIVOT_ROWS["negative"]], va[PIVOT_ROWS["nan"]], va[PIVOT_ROWS["zero"]] = -4.0, np.nan, 0.0
    return (VEC_ROWS,) + ed.diagonal_csr(va)


# ------------------------------------------------------------------------------------------ 2. sptrsv_csr_multi
MULTI_K = 9                                   # the second window, and at L = 64 the two halves of four
ORDERED_K = 5
MULTI_CASES = [(L, uplo, unit) for L in TRIP_LANES for uplo in (0, 1) for unit in (0, 1)]
ORDERED_CASES = [(0, 0), (1, 1)]              # (uplo, unit) of two_level_triangle(1, ...) under sptrsv_lanes=8


def multi_rhs(case, k):
    """(X, B, widest): k columns of integers in [-100, 100], B = T X in int64, and per column the largest
    sum_j |t_ij x_j| of a row (two_level_triangle's EXACT_LIMIT bound)"""
    n, rp, ci = case["n"], case["rp"], case["ci"]
    rng = np.random.default_rng([case["L"], case["uplo"], case["unit"], k])
    X = rng.integers(-100, 101, size=(n, k))
    rows = rows_of(n, rp)
    eff = np.where((rows == ci) & bool(case["unit"]), 1, case["va"].astype(np.int64))
    B = np.empty((n, k), np.int64)
    widest = np.empty(k, np.int64)
    for j in range(k):
        prod = (eff * X[ci, j]).astype(np.float64)                     # < 2^53: the sums below are exact
        B[:, j] = np.bincount(rows, weights=prod, minlength=n).astype(np.int64)
        widest[j] = int(np.bincount(rows, weights=np.abs(prod), minlength=n).max())
    return X.astype(np.float32), B.astype(np.float32), widest


# ------------------------------------------------------------------------------------------ 3. FSAI
# Slab<CLASS>::kFit and ::kWaves and groups_per_wave<CLASS, LANES>() of csrc/fsai.hip: whoever changes those moves
# the shapes below.
FSAI_FIT = {4: 96, 8: 32, 16: 9, 32: 2, 64: 1}
FSAI_WAVES = {4: 4, 8: 4, 16: 4, 32: 4, 64: 3}


def FSAI_ROWS_PER_BLOCK(cls, L):
    return min(64 // L, FSAI_FIT[cls]) * FSAI_WAVES[cls]


FSAI_TRIP_PAIRS = ((4, 64), (8, 64), (16, 8), (32, 16), (64, 1), (64, 64))
# "deep": long_first with 64 more rows, so that the second trip also reaches workgroups whose first-trip rows (row 63
# and below) all had the full length: there a slab holds a longest row first and a row of two entries next
FSAI_TRIP_CASES = [(cls, L, order) for cls, L in FSAI_TRIP_PAIRS for order in ("long_first", "short_first", "deep")]
FSAI_SHORT_BAND = 1
FSAI_DEEP_ROWS = fc.MAX_ROW


def fsai_trip_shape(cls, L, order):
    """(n, split, half-bandwidth before the split, after it)"""
    G = FSAI_ROWS_PER_BLOCK(cls, L)
    long_band = cls - 1                                                # b + 1 = class; 64 for class 64
    before, after = (FSAI_SHORT_BAND, long_band) if order == "short_first" else (long_band, FSAI_SHORT_BAND)
    return past_row_cap(L, G) + (FSAI_DEEP_ROWS if order == "deep" else 0), ROW_BLOCKS * G, before, after


def switched_band(n, split, before, after, seed=4):
    """symmetric diagonally dominant; row i stores (i, j), i - b <= j < i, b = `before` for i < split and `after` from
    there on, and the mirror of each"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    width = np.where(i < split, before, after)
    r = np.concatenate([i[(width >= dist) & (i >= dist)] for dist in range(1, max(before, after) + 1)])
    c = np.concatenate([i[(width >= dist) & (i >= dist)] - dist for dist in range(1, max(before, after) + 1)])
    v = rng.uniform(-1.0, 1.0, r.size).astype(np.float32)
    absv = np.abs(v).astype(np.float64)
    total = 1.0 + np.bincount(r, weights=absv, minlength=n) + np.bincount(c, weights=absv, minlength=n)
    return csr_from_coo(n, np.concatenate([r, c, i]), np.concatenate([c, r, i]),
                        np.concatenate([v, v, total.astype(np.float32)]))


def fsai_trip_matrix(cls, L, order):
    n, split, before, after = fsai_trip_shape(cls, L, order)
    return switched_band(n, split, before, after, seed=cls + L)


def rescaled(n, rp, ci, va):
    """new values on the same pattern; the symmetric scaling keeps the matrix SPD (test_gpu_fsai's refill)"""
    scale = (1.0 + 0.25 * np.sin(np.arange(n))).astype(np.float32)
    return (va * scale[rows_of(n, rp)] * scale[ci]).astype(np.float32)


FSAI_PERIOD = (6, 6, 5, 1, 6)                 # 24 rows
FSAI_PERIODS = 342                            # n = 8208 > 8192 = 2048 workgroups of 4 rows (class 8, 64 lanes)
FSAI_EXACT_LANES = 64


def fsai_exact_period():
    """(n0, rp0, ci0, va0, L0) of fsai_cases.exact_blocks(FSAI_PERIOD)"""
    return fc.exact_blocks(FSAI_PERIOD)


def repeat_blocks(n0, rp0, ci0, values, times):
    """the block-diagonal matrix of `times` copies of (n0, rp0, ci0, values)"""
    t = np.arange(times, dtype=np.int64)[:, None]
    rp = np.concatenate([[0], (np.asarray(rp0[1:], np.int64)[None, :] + t * int(rp0[-1])).ravel()]).astype(np.int32)
    ci = (np.asarray(ci0, np.int64)[None, :] + t * n0).ravel().astype(np.int32)
    return n0 * times, rp, ci, np.tile(np.asarray(values, np.float32), times)


def fsai_exact_matrix():
    n0, rp0, ci0, va0, _ = fsai_exact_period()
    return repeat_blocks(n0, rp0, ci0, va0, FSAI_PERIODS)


def fsai_exact_expected():
    """(g_rp, g_ci, g): one period proved by fsai_cases.prove_exact, repeated"""
    n0, rp0, ci0, va0, L0 = fsai_exact_period()
    g0 = fc.prove_exact(n0, rp0, ci0, va0, L0)
    g_rp0, g_ci0 = fc.lower_pattern(n0, rp0, ci0)
    return repeat_blocks(n0, g_rp0, g_ci0, g0, FSAI_PERIODS)[1:]


FSAI_DEFECT_ROWS = dict(unsorted=VEC_TRIP + 10, no_diagonal=VEC_TRIP + 20, wild_column=VEC_TRIP + 30,
                        long_row=VEC_TRIP + 200, bad_row=VEC_TRIP + 40)


def fsai_structure_matrix(defect=None):
    """tridiag(-1, 2, -1) of VEC_ROWS rows; with `defect`, its one flaw in row FSAI_DEFECT_ROWS[defect] >= VEC_TRIP"""
    n, rp, ci, va = tridiagonal(VEC_ROWS)
    if defect is None:
        return n, rp, ci, va
    r = FSAI_DEFECT_ROWS[defect]
    b, e = int(rp[r]), int(rp[r + 1])
    rp, ci, va = rp.copy(), ci.copy(), va.copy()
    if defect == "unsorted":                                           # (r, r) before (r, r - 1)
        ci[b], ci[b + 1], va[b], va[b + 1] = ci[b + 1], ci[b], va[b + 1], va[b]
    elif defect == "no_diagonal":
        ci, va = np.delete(ci, b + 1), np.delete(va, b + 1)
        rp[r + 1:] -= 1
    elif defect == "wild_column":                                      # the row's last column: it still ascends
        ci[e - 1] = n + 5
    elif defect == "long_row":                                         # 65 entries on and left of the diagonal
        new_ci = np.arange(r - fc.MAX_ROW, r + 2, dtype=np.int32)
        new_va = np.where(new_ci == r, 2.0, -0.01).astype(np.float32)
        ci = np.concatenate([ci[:b], new_ci, ci[e:]])
        va = np.concatenate([va[:b], new_va, va[e:]])
        rp[r + 1:] += new_ci.size - (e - b)
    elif defect == "bad_row":                                          # a negative diagonal: g_rr is a NaN
        va[b + 1] = -5.0
    else:
        raise KeyError(defect)
    return n, rp, ci, va


# ------------------------------------------------------------------------------------------ 4. AMG V-cycle
AMG_OMEGA = 0.5
# (n, forced amg_lanes or None, [(pre, coarse, post)])
AMG_CASES = {
    "L64": (2 * (row_trip(64) + 5), 64, [(1, 4, 1), (2, 2, 2), (2, 4, 0)]),
    "L8": (2 * (row_trip(8) + 33), 8, [(1, 4, 1)]),
    "vec": (2 * VEC_ROWS, None, [(1, 1, 1), (1, 4, 1)]),
}
AMG_TWIN_CHECKS = [(1, 4, 1), (2, 2, 2), (2, 4, 0), (1, 1, 1)]         # sweep counts of the (56, 28) comparison


class JacobiProver(ac.Prover):
    """amg_cases.Prover with separate pre / post sweep counts and, with coarse_sweeps given, the coarsest level solved
    by that many damped Jacobi sweeps from a zero guess (the Galerkin matrix of pair aggregates on tridiag(-1, 2, -1)
    is tridiag(-1, 2, -1) again, so wd = omega / 2 there as well: 1/4 at omega = 1/2)"""

    def cycle3(self, n, coarsest, f, omega, pre, post, coarse_sweeps=None):
        wd = Fraction(omega) / 2

        def from_zero(count):
            x = [self.total([wd * f[i]]) for i in range(n)]
            for _ in range(count - 1):
                x = self.sweep(n, wd, f, x)
            return x

        if n == coarsest:
            return self.cycle(n, n, f, omega, 1) if coarse_sweeps is None else from_zero(coarse_sweeps)
        x = from_zero(pre)
        fc_ = [self.total([self.residual(n, f, x, 2 * a), self.residual(n, f, x, 2 * a + 1)]) for a in range(n // 2)]
        e = self.cycle3(n // 2, coarsest, fc_, omega, pre, post, coarse_sweeps)
        x = [self.total([x[i], e[i // 2]]) for i in range(n)]
        for _ in range(post):
            x = self.sweep(n, wd, f, x)
        return x


def prove_vcycle_fractions(n, coarsest, r, omega, pre, post, coarse_sweeps=None):
    """(z as float32, bits) or (None, reason) by the Fraction prover"""
    prover = JacobiProver()
    try:
        z = prover.cycle3(n, coarsest, [Fraction(int(v)) for v in r], Fraction(omega), pre, post, coarse_sweeps)
    except ac.NotExact as why:
        return None, str(why)
    out = np.array([float(v) for v in z], np.float32)
    assert all(Fraction(float(a)) == b for a, b in zip(out, z))
    return out, prover.bits


class FastProver:
    """The same cycle and the same rule in int64 fixed point, a vector at a time.  A value v is the integer
    v * 2^SHIFT.  total() takes the terms of one sum per element: their common quantum q is the lowest set bit of any
    of them (at most 1: the Fraction prover's scale starts at 1), and the sum is admitted when sum |terms| < 2^24 q."""
    SHIFT = 32                                # finer values are refused (scaled)

    def __init__(self):
        self.bits = 0

    def total(self, *terms):
        t = np.stack(np.broadcast_arrays(*terms))
        mag = np.abs(t)
        if int(mag.max(initial=0)) >= 1 << 58:                         # 2^26 quanta or more (q <= 1); int64 holds the rest
            raise ac.NotExact("a term of 2^%d" % (int(mag.max()).bit_length() - 1 - self.SHIFT))
        low = np.bitwise_or.reduce(mag, axis=0)
        quantum = np.where(low == 0, 1 << self.SHIFT, np.minimum(low & -low, 1 << self.SHIFT))
        units = int((mag.sum(axis=0) // quantum).max(initial=0))
        self.bits = max(self.bits, units.bit_length())
        if units >= EXACT_LIMIT:
            raise ac.NotExact("a sum needs %d bits" % units.bit_length())
        return t.sum(axis=0)

    @staticmethod
    def scaled(v, wd_shift):
        """wd * v, wd = 2^-wd_shift; the fixed point must hold the result"""
        if (v & ((1 << wd_shift) - 1)).any():
            raise ac.NotExact("finer than 2^-%d" % FastProver.SHIFT)
        return v >> wd_shift

    def residual(self, f, x):
        left, right = np.zeros_like(x), np.zeros_like(x)
        left[1:], right[:-1] = x[:-1], x[1:]
        return self.total(f, -2 * x, left, right)

    def sweep(self, wd_shift, f, x):
        return self.total(self.scaled(self.residual(f, x), wd_shift), x)

    def from_zero(self, wd_shift, f, count):
        x = self.total(self.scaled(f, wd_shift))
        for _ in range(count - 1):
            x = self.sweep(wd_shift, f, x)
        return x

    def dense(self, f):
        """the stored inverse of tridiag(-1, 2, -1) times f, by the Fraction prover on the few rows of this level"""
        small = ac.Prover()
        z = small.cycle(f.size, f.size, [Fraction(int(v), 1 << self.SHIFT) for v in f], Fraction(1), 1)
        self.bits = max(self.bits, small.bits)
        out = [v * (1 << self.SHIFT) for v in z]
        if any(v.denominator != 1 for v in out):
            raise ac.NotExact("finer than 2^-%d" % self.SHIFT)
        return np.array([int(v) for v in out], np.int64)

    def cycle(self, n, coarsest, f, wd_shift, pre, post, coarse_sweeps):
        assert f.size == n
        if n == coarsest:
            return self.dense(f) if coarse_sweeps is None else self.from_zero(wd_shift, f, coarse_sweeps)
        x = self.from_zero(wd_shift, f, pre)
        res = self.residual(f, x)
        coarse = self.total(res[0::2], res[1::2])
        e = self.cycle(n // 2, coarsest, coarse, wd_shift, pre, post, coarse_sweeps)
        x = self.total(x, np.repeat(e, 2))
        for _ in range(post):
            x = self.sweep(wd_shift, f, x)
        return x


def prove_vcycle_fast(n, coarsest, r, omega, pre, post, coarse_sweeps=None):
    """(z as float32, bits) when every intermediate of the cycle is exact in fp32, else (None, reason)"""
    wd = Fraction(omega) / 2
    assert wd.numerator == 1 and wd.denominator & (wd.denominator - 1) == 0
    prover = FastProver()
    f = np.asarray(r, np.float64)
    assert (f == np.rint(f)).all()
    try:
        z = prover.cycle(n, coarsest, np.rint(f).astype(np.int64) << prover.SHIFT, wd.denominator.bit_length() - 1,
                         pre, post, coarse_sweeps)
    except ac.NotExact as why:
        return None, str(why)
    exact = z.astype(np.float64) / float(1 << prover.SHIFT)            # |z| < 2^53 units: the quotient is exact
    assert (np.abs(z) < 1 << 53).all()
    out = exact.astype(np.float32)
    assert (out.astype(np.float64) == exact).all()
    return out, prover.bits


# ------------------------------------------------------------------------------------------ 5. AMG setup on the device
MIS_CAP_GRID = 96                            # poisson2d(96): 9216 rows, 2304 workgroups of 4 rows asked for at 64 lanes
MIS_L8_GRID = 257                             # poisson2d(257): 66 049 rows, just past row_trip(8)
MIS_SEEDS = (0, 0xDEADBEEF)
SETUP_BAD_ROW = VEC_TRIP + 77                 # the zero diagonal of the rejected variant: the second trip of workgroup 0
SETUP_LAST_PARTIAL_ROW = VEC_TRIP - 3         # and of a second one: workgroup 1023, the last partial min_fold_kernel reads


# ------------------------------------------------------------------------------------------ 6. smoothed AMG V-cycle
SMOOTHED_WEIGHT = 1.0                         # omega_p: at 1/2 the coarse diagonal is 5/8 and the cycle rounds
# name: (n, forced amg_lanes or None, [(pre, coarse, post)]).  A has n rows, P has n, PT and level 1 have n / 2.
# "below", "at" and "above" put PT's rows one under, at and one over row_trip(64) while A and P are in their third trip.
# Nothing had to be narrowed to be admitted: the right-hand side is amg_cases.exact_rhs (integers in [-8, 8]) and the
# widest sum of any case takes 18 bits (the host test prints them).
SMOOTHED_CASES = {
    "L64": (2 * (row_trip(64) + 5), 64, [(1, 1, 1), (2, 2, 2), (2, 4, 0)]),
    "L8": (2 * (row_trip(8) + 33), 8, [(1, 4, 1)]),
    "below": (2 * (row_trip(64) - 1), 64, [(1, 1, 1)]),
    "at": (2 * row_trip(64), 64, [(1, 1, 1)]),
    "above": (2 * (row_trip(64) + 1), 64, [(1, 1, 1)]),
    "vec": (2 * VEC_ROWS, None, [(1, 1, 1), (2, 4, 0)]),
}
SMOOTHED_TWIN_ROWS = 2 * (ac.DENSE_ROWS + 8)  # the smallest family member whose coarsest level is Jacobi-solved
SMOOTHED_TWIN_CHECKS = [(1, 1, 1), (2, 2, 2), (2, 4, 0), (1, 4, 1)]    # sweep counts of the comparison with Fractions


def dyadic(values):
    """(ints, shift) with values == ints * 2^-shift exactly, for the smallest shift up to 30"""
    v = np.asarray(values, np.float64)
    for shift in range(31):
        scaled = v * float(1 << shift)
        if (scaled == np.rint(scaled)).all():
            ints = np.rint(scaled).astype(np.int64)
            if int(np.abs(ints).max(initial=0)) >= 1 << 30:
                break
            return ints, shift
    raise ac.NotExact("a coefficient is no short dyadic number")


class SmoothedProver(FastProver):
    """FastProver's fixed point and rule for the weighted cycle on level matrices, P and PT given as CSR arrays: no
    closed form.  A coefficient (a matrix entry, wd_i) is an integer times 2^-shift (dyadic); a product with a value
    must stay inside the fixed point.  row_total() is total() for the sums of a row sweep, one sum per row: the
    terms are the row's products and, where the kernel's epilogue adds one, the row's own term (f_i of the residual,
    x_i of the prolongation).  The dot product and the epilogue are held as ONE sum, which covers both."""

    @staticmethod
    def times(coefficient, v):
        ints, shift = coefficient
        if int(np.abs(ints).max(initial=0)).bit_length() + int(np.abs(v).max(initial=0)).bit_length() > 62:
            raise ac.NotExact("a product past int64")
        product = ints * v
        if (product & ((1 << shift) - 1)).any():
            raise ac.NotExact("finer than 2^-%d" % FastProver.SHIFT)
        return product >> shift

    @staticmethod
    def matrix(rows, csr):
        rp, ci, va = csr
        rp = np.asarray(rp, np.int64)
        assert rp.size == rows + 1 and rp[0] == 0 and rp[-1] == len(ci) and (np.diff(rp) >= 0).all()
        return dict(rows=rows, rp=rp, ci=np.asarray(ci, np.int64), va=dyadic(va), full=rp[1:] > rp[:-1])

    def row_total(self, M, x, own=None, sign=1):
        """per row i: own_i + sign * sum_j m_ij x_j, every row's sum admitted by total()'s rule"""
        terms = sign * self.times(M["va"], x[M["ci"]])
        mag = np.abs(terms)
        starts = M["rp"][:-1][M["full"]]
        total, size, low = (np.zeros(M["rows"], np.int64) for _ in range(3))
        if terms.size:
            total[M["full"]] = np.add.reduceat(terms, starts)
            size[M["full"]] = np.add.reduceat(mag, starts)
            low[M["full"]] = np.bitwise_or.reduceat(mag, starts)
        if own is not None:
            total, size, low = total + own, size + np.abs(own), low | np.abs(own)
        if int(size.max(initial=0)) >= 1 << 58:
            raise ac.NotExact("a row of 2^%d" % (int(size.max()).bit_length() - 1 - self.SHIFT))
        quantum = np.where(low == 0, 1 << self.SHIFT, np.minimum(low & -low, 1 << self.SHIFT))
        units = int((size // quantum).max(initial=0))
        self.bits = max(self.bits, units.bit_length())
        if units >= EXACT_LIMIT:
            raise ac.NotExact("a sum needs %d bits" % units.bit_length())
        return total

    # the three kernels of a smoothed level
    def residual_of(self, A, f, x):
        return self.row_total(A, x, own=f, sign=-1)

    def restricted(self, PT, res):
        return self.row_total(PT, res)

    def prolonged(self, P, x, e):
        return self.row_total(P, e, own=x)

    def jacobi(self, A, wd, f, count):
        """`count` damped Jacobi sweeps from a zero guess: wd_i f_i, then fmaf(wd_i, f_i - (A x)_i, x_i)"""
        x = self.total(self.times(wd, f))
        for _ in range(count - 1):
            x = self.total(self.times(wd, self.residual_of(A, f, x)), x)
        return x

    def smoothed_cycle(self, levels, l, f, omega, pre, post, coarse_sweeps):
        level = levels[l]
        n = level["n"]
        assert f.size == n
        A = self.matrix(n, (level["rp"], level["ci"], level["va"]))
        d = ac.diag32(n, level["rp"], level["ci"], level["va"]).astype(np.float64)
        wd = dyadic((np.float64(np.float32(omega)) / d).astype(np.float32))       # the fp32 array the library stores
        if l == len(levels) - 1:
            if n <= ac.DENSE_ROWS:
                raise ac.NotExact("a dense coarsest level")
            return self.jacobi(A, wd, f, coarse_sweeps)
        P, PT = self.matrix(n, level["P"]), self.matrix(level["count"], level["PT"])
        x = self.jacobi(A, wd, f, pre)
        coarse = self.restricted(PT, self.residual_of(A, f, x))
        e = self.smoothed_cycle(levels, l + 1, coarse, omega, pre, post, coarse_sweeps)
        x = self.prolonged(P, x, e)
        for _ in range(post):
            x = self.total(self.times(wd, self.residual_of(A, f, x)), x)
        return x

    def as_float32(self, v):
        assert (np.abs(v) < 1 << 53).all()
        exact = v.astype(np.float64) / float(1 << self.SHIFT)          # |v| < 2^53 units: the quotient is exact
        out = exact.astype(np.float32)
        assert (out.astype(np.float64) == exact).all()
        return out

    def fixed(self, vector):
        v = np.asarray(vector, np.float64)
        assert (v == np.rint(v)).all()
        return np.rint(v).astype(np.int64) << self.SHIFT


def prove_smoothed_vcycle_fast(levels, r, omega, pre, post, coarse_sweeps):
    """(z as float32, bits) when every sum of the weighted cycle on `levels` (amg_smoothed_cases.hierarchy's dicts, or
    what the device gives back in that form) is exact in fp32 whatever order the lanes take, else (None, reason):
    the Jacobi sweeps, r = f - A x, PT r, the coarse sweeps from a zero guess, x + P e and the post-sweeps."""
    prover = SmoothedProver()
    try:
        z = prover.smoothed_cycle(levels, 0, prover.fixed(r), omega, pre, post, coarse_sweeps)
    except ac.NotExact as why:
        return None, str(why)
    return prover.as_float32(z), prover.bits


def prove_smoothed_transfers_fast(level, f, x, e):
    """amg_smoothed_cases.prove_transfers, vectorised, with the residual as well: (residual, f_coarse, x_out, bits)
    as float32 arrays, or (None, None, None, reason)"""
    prover = SmoothedProver()
    n, count = level["n"], level["count"]
    try:
        A = prover.matrix(n, (level["rp"], level["ci"], level["va"]))
        res = prover.residual_of(A, prover.fixed(f), prover.fixed(x))
        coarse = prover.restricted(prover.matrix(count, level["PT"]), res)
        out = prover.prolonged(prover.matrix(n, level["P"]), prover.fixed(x), prover.fixed(e))
    except ac.NotExact as why:
        return None, None, None, str(why)
    return prover.as_float32(res), prover.as_float32(coarse), prover.as_float32(out), prover.bits


def smoothed_hierarchy(spmv, n):
    """tridiag(-1, 2, -1) of n rows, pair aggregates, omega_p = 1: the two levels through the host twins"""
    return sc.hierarchy(spmv, *tridiagonal(n), maps=ac.pair_maps(n, n // 2), weight=SMOOTHED_WEIGHT)


class SmoothedFractions(ac.Prover):
    """The same cycle by amg_cases.Prover's total() on Fractions, a row at a time: what SmoothedProver is held to"""

    def sweep_rows(self, rows, x, own=None, sign=1):
        return [self.total(([own[i]] if own is not None else []) + [sign * a * x[j] for j, a in row])
                for i, row in enumerate(rows)]

    def jacobi(self, A, wd, f, count):
        x = [self.total([w * v]) for w, v in zip(wd, f)]
        for _ in range(count - 1):
            x = [self.total([w * r, v]) for w, r, v in zip(wd, self.sweep_rows(A, x, f, -1), x)]
        return x

    def smoothed_cycle(self, levels, l, f, omega, pre, post, coarse_sweeps):
        level = levels[l]
        n = level["n"]
        A = sc._rows(n, (level["rp"], level["ci"], level["va"]))
        d = ac.diag32(n, level["rp"], level["ci"], level["va"]).astype(np.float64)
        wd = [Fraction(float(w)) for w in (np.float64(np.float32(omega)) / d).astype(np.float32)]
        if l == len(levels) - 1:
            assert n > ac.DENSE_ROWS
            return self.jacobi(A, wd, f, coarse_sweeps)
        x = self.jacobi(A, wd, f, pre)
        coarse = self.sweep_rows(sc._rows(level["count"], level["PT"]), self.sweep_rows(A, x, f, -1))
        e = self.smoothed_cycle(levels, l + 1, coarse, omega, pre, post, coarse_sweeps)
        x = self.sweep_rows(sc._rows(n, level["P"]), e, x)
        for _ in range(post):
            x = [self.total([w * r, v]) for w, r, v in zip(wd, self.sweep_rows(A, x, f, -1), x)]
        return x


def prove_smoothed_vcycle_fractions(levels, r, omega, pre, post, coarse_sweeps):
    """(z as float32, bits) or (None, reason) by the Fraction prover"""
    prover = SmoothedFractions()
    try:
        z = prover.smoothed_cycle(levels, 0, [Fraction(int(v)) for v in r], omega, pre, post, coarse_sweeps)
    except ac.NotExact as why:
        return None, str(why)
    out = np.array([float(v) for v in z], np.float32)
    assert all(Fraction(float(a)) == b for a, b in zip(out, z))
    return out, prover.bits
