"""Matrices and restatements shared by the FSAI tests (test_fsai_host.py, test_gpu_fsai.py, test_gpu_cg_fsai.py).

* numpy_fsai: the arithmetic of include/spmv/fsai.h restated entry by entry in fp64.  The fused multiply-add is taken
  in exact rational arithmetic (fractions.Fraction) and rounded once, so there is no double rounding anywhere; the
  square root and the quotient are numpy's correctly rounded fp64 operations, the store one rounding to fp32.
* exact_blocks / prove_exact: block-diagonal A = L L^T with dense blocks and dyadic L (small integers below a
  power-of-two diagonal).  The pattern holds everything, so G = L^-1 exactly; prove_exact runs the rule in Fractions,
  asserts that every Cholesky and substitution intermediate is representable in fp64 (no operation rounds) and that each
  g fits fp32, and that the result is the Fraction inverse of L.
* dense_spd_block / banded_spd / mixed_rows / the pattern helpers: inexact shapes for the host and device tests.
"""
import math
from fractions import Fraction

import numpy as np

from ilu0_cases import csr_from_coo, rows_of  # noqa: F401  (rows_of is used by the tests)

MAX_ROW = 64          # include/spmv/fsai.h kFsaiMaxRow
CLASSES = (4, 8, 16, 32, 64)


def class_for(max_row):
    return next(c for c in CLASSES if max_row <= c)


def fma64(a, b, c):
    """fma(a, b, c) in fp64 with one rounding; non-finite operands take the IEEE result of the separate operations
    (NaN / inf propagate the same way: only whether the result is finite is compared for them)"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # an exact zero is -0 only as the sum of a zero product and a zero addend that are both negative; x + (-x) is +0
        both_zero = (a == 0 or b == 0) and c == 0
        negative = math.copysign(1.0, a) * math.copysign(1.0, b) < 0 and math.copysign(1.0, c) < 0
        return -0.0 if both_zero and negative else 0.0
    return float(exact)


def lower_pattern(n, rp, ci):
    """(g_rp, g_ci): the columns j <= i of every row"""
    rows = rows_of(n, rp)
    keep = np.asarray(ci, np.int64) <= rows
    g_rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return g_rp, np.asarray(ci, np.int32)[keep]


def fsai_row(where, pattern):
    """u (fp64 list) of one row by the rule of fsai.h; where[j] maps column -> fp32 value of row j of A"""
    m = len(pattern)
    M = [[0.0] * (p + 1) for p in range(m)]
    for p in range(m):
        row = where[pattern[p]]
        for q in range(p + 1):
            v = row.get(pattern[q])
            if v is not None:
                M[p][q] = float(v)
    C = M
    with np.errstate(all="ignore"):
        for q in range(m):
            for p in range(q, m):
                w = C[p][q]
                for k in range(q):
                    w = fma64(-C[p][k], C[q][k], w)
                if p == q:
                    C[q][q] = float(np.sqrt(np.float64(w)))
                else:
                    C[p][q] = float(np.float64(w) / np.float64(C[q][q]))
        u = [0.0] * m
        u[m - 1] = float(np.float64(1.0) / np.float64(C[m - 1][m - 1]))
        for p in range(m - 2, -1, -1):
            t = 0.0
            for q in range(m - 1, p, -1):
                t = fma64(C[q][p], u[q], t)
            u[p] = float(np.float64(-t) / np.float64(C[p][p]))
    return u


def numpy_fsai(n, rp, ci, va, pattern=None):
    """(g_rp, g_ci, g_values fp32, bad_row) by the rule of fsai.h; pattern = (s_rp, s_ci) or None for A's own"""
    s_rp, s_ci = (rp, ci) if pattern is None else pattern
    g_rp, g_ci = lower_pattern(n, s_rp, s_ci)
    va = np.asarray(va, np.float32)
    where = [{int(ci[t]): va[t] for t in range(rp[j], rp[j + 1]) if ci[t] <= j} for j in range(n)]
    g = np.empty(g_ci.size, np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            b, e = int(g_rp[i]), int(g_rp[i + 1])
            assert e > b and g_ci[e - 1] == i
            g[b:e] = np.asarray(fsai_row(where, [int(c) for c in g_ci[b:e]]), np.float64).astype(np.float32)
    d = g[g_rp[1:] - 1]
    bad = np.flatnonzero(~((d > 0) & np.isfinite(d)))
    return g_rp, g_ci, g, (int(bad[0]) if bad.size else -1)


# ---- the exact tier -------------------------------------------------------------------------------------------
def _fits(x, bits):
    """the Fraction x is a binary floating-point number with a `bits`-bit significand (exponent range not an issue)"""
    if x == 0:
        return True
    d = x.denominator
    if d & (d - 1):
        return False
    num = abs(x.numerator)
    while num % 2 == 0:
        num //= 2
    return num.bit_length() <= bits


def exact_blocks(sizes, seed=3):
    """Block-diagonal A = L L^T, one dense block per entry of `sizes`; L has a diagonal drawn from {1, 2, 4} and
    integers from {-1, 0, 1} below it.  Returns (n, rp, ci, va, L) with L the dense integer factor."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    L = np.zeros((n, n), np.int64)
    block = np.zeros((n, n), bool)
    at = 0
    for m in sizes:
        blk = np.tril(rng.integers(-1, 2, (m, m)), -1)
        blk[np.arange(m), np.arange(m)] = rng.choice([1, 2, 4], m)
        L[at:at + m, at:at + m] = blk
        block[at:at + m, at:at + m] = True
        at += m
    A = L @ L.T
    rows, cols = np.nonzero(block)                            # the blocks, whole: a zero of A inside one is stored
    n, rp, ci, va = csr_from_coo(n, rows, cols, A[rows, cols].astype(np.float32))
    return n, rp, ci, va, L


def prove_exact(n, rp, ci, va, L):
    """Runs the rule of fsai.h on A's own lower pattern in Fractions.  Asserts that A's stored values are L L^T, that
    every Cholesky and substitution intermediate is an fp64 number (so no operation rounds), that every u fits fp32,
    and that G is the exact inverse of L.  Returns G's values (fp32) in the lower pattern's order."""
    g_rp, g_ci = lower_pattern(n, rp, ci)
    A = L @ L.T
    for i in range(n):
        for t in range(rp[i], rp[i + 1]):
            assert float(va[t]) == float(A[i, ci[t]])
    Lf = [[Fraction(int(v)) for v in row] for row in L]
    inverse = [[Fraction(0)] * n for _ in range(n)]           # forward substitution, column by column
    for c in range(n):
        for i in range(c, n):
            s = Fraction(1 if i == c else 0) - sum(Lf[i][k] * inverse[k][c] for k in range(c, i))
            inverse[i][c] = s / Lf[i][i]
    out = np.empty(g_ci.size, np.float32)
    for i in range(n):
        P = [int(c) for c in g_ci[g_rp[i]:g_rp[i + 1]]]
        m = len(P)
        assert P[-1] == i
        C = [[Fraction(int(A[P[p], P[q]])) for q in range(p + 1)] for p in range(m)]
        for q in range(m):
            for p in range(q, m):
                w = C[p][q]
                for k in range(q):
                    w = w - C[p][k] * C[q][k]
                    assert _fits(w, 53)
                if p == q:
                    root = math.isqrt(int(w))
                    assert w > 0 and w.denominator == 1 and root * root == w
                    C[q][q] = Fraction(root)
                else:
                    C[p][q] = w / C[q][q]
                    assert _fits(C[p][q], 53)
        u = [Fraction(0)] * m
        u[m - 1] = 1 / C[m - 1][m - 1]
        for p in range(m - 2, -1, -1):
            t = Fraction(0)
            for q in range(m - 1, p, -1):
                t = t + C[q][p] * u[q]
                assert _fits(t, 53)
            u[p] = -t / C[p][p]
        for p in range(m):
            assert _fits(u[p], 24) and u[p] == inverse[i][P[p]], (i, p)
            # a zero is the rule's (-t) / c_pp with t = +0.0 (an exact zero sum is +0 in round-to-nearest): -0.0
            out[g_rp[i] + p] = np.float32(float(u[p])) if u[p] != 0 else np.float32(-0.0)
        outside = [c for c in range(i + 1) if c not in P]
        assert all(inverse[i][c] == 0 for c in outside)
    return out


# ---- inexact shapes -----------------------------------------------------------------------------------------------
def _dominant(dense):
    dense = (dense + dense.T) / 2
    np.fill_diagonal(dense, 0.0)
    np.fill_diagonal(dense, np.abs(dense).sum(axis=1) + 1.0)
    return dense


def dense_spd_block(m, seed=2):
    """one dense m x m symmetric diagonally dominant matrix: its lower pattern has rows of every length 1 .. m"""
    dense = _dominant(np.random.default_rng(seed).uniform(-1.0, 1.0, (m, m)))
    rows, cols = np.nonzero(np.ones((m, m)))
    return csr_from_coo(m, rows, cols, dense[rows, cols].astype(np.float32))


def banded_spd(n, b, seed=4):
    """symmetric diagonally dominant with every entry |i - j| <= b stored: the longest pattern row has b + 1 entries"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    off = {}
    for i in range(n):
        for j in range(max(0, i - b), i):
            off[(i, j)] = rng.uniform(-1.0, 1.0)
    total = np.ones(n)
    for (i, j), v in off.items():
        total[i] += abs(v)
        total[j] += abs(v)
    for i in range(n):
        for j in range(max(0, i - b), min(n, i + b + 1)):
            rows.append(i), cols.append(j)
            vals.append(total[i] if i == j else off[(max(i, j), min(i, j))])
    return csr_from_coo(n, rows, cols, np.asarray(vals, np.float32))


def mixed_rows(groups=6, seed=6):
    """dense 64 x 64 blocks separated by runs of 40 diagonal-only rows: rows of length 1 and of length up to 64 meet
    in one wavefront's groups at every lane count"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    at = 0
    for _ in range(groups):
        for i in range(40):
            rows.append(at + i), cols.append(at + i), vals.append(rng.uniform(1.0, 3.0))
        at += 40
        dense = _dominant(rng.uniform(-1.0, 1.0, (64, 64)))
        for i in range(64):
            for j in range(64):
                rows.append(at + i), cols.append(at + j), vals.append(dense[i, j])
        at += 64
    return csr_from_coo(at, rows, cols, np.asarray(vals, np.float32))


def identity_pattern(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def band_of(n, rp, ci, width):
    """the stored entries of the pattern with |i - j| <= width"""
    rows = rows_of(n, rp)
    keep = np.abs(np.asarray(ci, np.int64) - rows) <= width
    s_rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return s_rp, np.asarray(ci, np.int32)[keep]


def squared_pattern(n, rp, ci):
    """the pattern of A*A (every structural product counts), rows ascending"""
    neighbours = [set(int(c) for c in ci[rp[i]:rp[i + 1]]) for i in range(n)]
    s_rp, s_ci = [0], []
    for i in range(n):
        reach = set()
        for k in neighbours[i]:
            reach |= neighbours[k]
        s_ci.extend(sorted(reach))
        s_rp.append(len(s_ci))
    return np.asarray(s_rp, np.int32), np.asarray(s_ci, np.int32)


def indefinite(n=40, row=17):
    """banded_spd(n, 3) with one diagonal made negative: the rows from `row` on that hold it in their pattern go bad"""
    n, rp, ci, va = banded_spd(n, 3)
    va = va.copy()
    va[(rows_of(n, rp) == row) & (ci == row)] = -5.0
    return n, rp, ci, va


def unit_diagonal_error(n, rp, ci, va, g_rp, g_ci, g):
    """max |diag(G A G^T) - 1| in fp64, A symmetrised from its lower triangle"""
    A = np.zeros((n, n))
    rows = rows_of(n, rp)
    low = np.asarray(ci) <= rows
    A[rows[low], np.asarray(ci)[low]] = np.asarray(va, np.float64)[low]
    A = A + np.tril(A, -1).T
    G = np.zeros((n, n))
    G[rows_of(n, g_rp), g_ci] = np.asarray(g, np.float64)
    return float(np.abs(np.einsum("ij,jk,ik->i", G, A, G) - 1.0).max())
