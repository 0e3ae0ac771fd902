"""Matrices and restatements shared by the IC(0) tests (test_ic0_host.py, test_gpu_ic0.py, test_gpu_cg_ic.py).

* numpy_ic0: the arithmetic of include/spmv/ic0.h restated entry by entry, the fma taken as the fp64 product and
  difference rounded once to fp32 (the product of two fp32 values is exact in fp64; where the fp64 sum is itself
  rounded the tests' values are far from a double-rounding tie, and the exact cases below do not round at all), the
  square root np.sqrt on float32 (correctly rounded).
* exact_tridiagonal / arrow_spd: dyadic matrices whose pattern holds all the fill and whose pivots are perfect
  squares, so IC(0) is the exact Cholesky factor; prove_exact runs the recurrence in integer fixed point, checks that
  every quotient, update and square root is exact and representable in fp32, and that L L^T == A entry for entry, and
  returns the factor's values in A's pattern (L^T in the upper positions).
* sorted_random_spd / spd_blocks: inexact shapes for the device tests.
"""
import math

import numpy as np

from ilu0_cases import csr_from_coo, fma32, rows_of  # noqa: F401  (rows_of is used by the tests)


def _diagonal_positions(n, rp, ci):
    diag = np.full(n, -1, np.int64)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                diag[i] = j
    assert (diag >= 0).all()
    return diag


def numpy_ic0(n, rp, ci, va):
    """(l_values, bad_pivot) by the rule of ic0.h; rows strictly ascending, every diagonal stored, a structurally
    symmetric pattern.  Only A's lower triangle and diagonal are read; the upper positions receive L^T."""
    va = np.asarray(va, np.float32)
    l = np.full(va.size, np.nan, np.float32)
    diag = _diagonal_positions(n, rp, ci)
    where = [{int(ci[q]): q for q in range(rp[k], rp[k + 1])} for k in range(n)]
    with np.errstate(all="ignore"):
        for i in range(n):
            di = diag[i]
            l[rp[i]:di + 1] = va[rp[i]:di + 1]
            for pk in range(rp[i], di):
                k = int(ci[pk])
                lik = np.float32(l[pk] / l[diag[k]])
                l[pk] = lik
                for t in range(pk + 1, di):
                    q = where[k].get(int(ci[t]))            # (k,j) holds l_jk
                    if q is not None:
                        l[t] = fma32(-lik, l[q], l[t])
                l[di] = fma32(-lik, lik, l[di])
                l[where[k][i]] = lik                         # the mirror store to (k,i)
            l[di] = np.sqrt(l[di])
    d = l[diag]
    bad = np.flatnonzero(~((d > 0) & np.isfinite(d)))
    return l, (int(bad[0]) if bad.size else -1)


def prove_exact(n, rp, ci, va, shift=0):
    """IC(0) of (n, rp, ci, va) in integer fixed point with `shift` fractional bits.  Asserts that A's lower values
    are multiples of 2^-shift, that every quotient, update and square root is exact and below 2^24 units (so fp32
    holds it and no operation rounds), and that L L^T == A on and off the pattern of the lower triangle (IC(0) is the
    exact Cholesky factor).  Returns the factor in A's pattern, L^T in the upper positions."""
    one = 1 << shift
    a = np.asarray(va, np.float64) * one
    w = np.rint(a).astype(np.int64)
    diag = _diagonal_positions(n, rp, ci)
    lower = rows_of(n, rp) >= np.asarray(ci, np.int64)
    assert (w == a)[lower].all()
    w = [int(v) for v in w]
    where = [{int(ci[q]): q for q in range(rp[k], rp[k + 1])} for k in range(n)]
    for i in range(n):
        assert (np.diff(ci[rp[i]:rp[i + 1]]) > 0).all()
        for j in ci[rp[i]:rp[i + 1]]:
            assert i in where[int(j)], (i, j)                # structurally symmetric
    limit = 1 << 24
    for i in range(n):
        di = int(diag[i])
        for pk in range(rp[i], di):
            k = int(ci[pk])
            num, den = w[pk] * one, w[diag[k]]
            assert den > 0 and num % den == 0
            lik = num // den
            assert abs(lik) < limit
            w[pk] = lik
            for t in range(pk + 1, di):
                q = where[k].get(int(ci[t]))
                if q is not None:
                    prod = lik * w[q]
                    assert prod % one == 0
                    w[t] -= prod // one
                    assert abs(w[t]) < limit
            assert (lik * lik) % one == 0
            w[di] -= lik * lik // one
            assert abs(w[di]) < limit
            w[where[k][i]] = lik
        assert w[di] > 0
        root = math.isqrt(w[di] * one)                       # sqrt(w / one) = root / one
        assert root * root == w[di] * one and root < limit
        w[di] = root
    # L L^T == A on the lower triangle, and nothing outside its pattern
    rows = [{int(ci[p]): w[p] for p in range(rp[i], diag[i] + 1)} for i in range(n)]
    by_column = {}
    for i in range(n):
        for k in rows[i]:
            by_column.setdefault(k, []).append(i)
    acc = {}
    for k, members in by_column.items():
        for i in members:
            for j in members:
                if j <= i:
                    acc[(i, j)] = acc.get((i, j), 0) + rows[i][k] * rows[j][k]
    want = {(i, int(ci[p])): int(round(float(va[p]) * one)) * one for i in range(n) for p in range(rp[i], diag[i] + 1)}
    for key, v in acc.items():
        assert v == want.get(key, 0), key
    for key, v in want.items():
        assert acc.get(key, 0) == v, key
    l = (np.array(w, np.float64) / one).astype(np.float32)
    assert (l.astype(np.float64) * one == np.array(w, np.float64)).all()
    return l


def exact_tridiagonal(n, seed=0):
    """A = L L^T with L lower bidiagonal: diagonal d_i drawn from {1, 2, 4, 8}, sub-diagonal e_i a non-zero integer
    with |e_i| <= min(2, d_i) (no row of L lets the forward substitution grow).  Returns (n, rp, ci, va, fact) with
    fact the factor in A's pattern."""
    rng = np.random.default_rng(seed)
    d = rng.choice([1, 2, 4, 8], n)
    e = rng.choice([-2, -1, 1, 2], n)
    e = np.sign(e) * np.minimum(np.abs(e), d)
    rows, cols, vals, fact = [], [], [], []
    for i in range(n):
        if i > 0:
            rows.append(i), cols.append(i - 1), vals.append(e[i] * d[i - 1]), fact.append(e[i])
        rows.append(i), cols.append(i), vals.append(d[i] * d[i] + (e[i] * e[i] if i > 0 else 0)), fact.append(d[i])
        if i + 1 < n:
            rows.append(i), cols.append(i + 1), vals.append(e[i + 1] * d[i]), fact.append(e[i + 1])
    n, rp, ci, va = csr_from_coo(n, rows, cols, vals)          # (already in order)
    return n, rp, ci, va, np.array(fact, np.float32)


def arrow_spd(n, seed=7):
    """diagonal drawn from {1, 4, 16, 64} (powers of two with an exact root), an integer last row and column, and the
    corner = sum_i a_i^2 / d_i + 64^2: large enough that the last pivot stays positive, and the perfect square 64^2
    after the updates.  The factor's values are multiples of 1/8 and the running corner of 1/64: prove with shift=6."""
    rng = np.random.default_rng(seed)
    d = rng.choice([1, 4, 16, 64], n - 1)
    a = rng.integers(-4, 5, n - 1)
    a[a == 0] = 1
    corner = float(np.sum(a.astype(np.float64) ** 2 / d)) + 64.0 ** 2
    rows, cols, vals = [], [], []
    for i in range(n - 1):
        rows += [i, i]
        cols += [i, n - 1]
        vals += [d[i], a[i]]
    rows += [n - 1] * n
    cols += list(range(n))
    vals += list(a) + [corner]
    return csr_from_coo(n, rows, cols, vals)


def sorted_random_spd(n, per_row, seed):
    """symmetric, strictly diagonally dominant with a positive diagonal (hence SPD), about per_row stored entries per
    row, columns de-duplicated and ascending"""
    rng = np.random.default_rng(seed)
    half = max((per_row - 1) // 2, 1)
    r = np.repeat(np.arange(n, dtype=np.int64), half)
    c = rng.integers(0, n, r.size)
    keep = r != c
    lo, hi = np.minimum(r, c)[keep], np.maximum(r, c)[keep]
    pairs = np.unique(lo * n + hi)
    lo, hi = pairs // n, pairs % n
    v = rng.uniform(-1.0, 1.0, pairs.size).astype(np.float32)
    absv = np.abs(v).astype(np.float64)
    d = np.bincount(lo, weights=absv, minlength=n) + np.bincount(hi, weights=absv, minlength=n) + 1.0
    rows = np.concatenate([lo, hi, np.arange(n)])
    cols = np.concatenate([hi, lo, np.arange(n)])
    vals = np.concatenate([v, v, d.astype(np.float32)])
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return n, rp, cols[order].astype(np.int32), vals[order].astype(np.float32)


def spd_blocks(blocks, seed=5):
    """`blocks` independent dense 3 x 3 symmetric diagonally dominant blocks: three levels, each `blocks` rows wide"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for b in range(blocks):
        m = rng.uniform(-1.0, 1.0, (3, 3))
        m = (m + m.T) / 2
        m[np.arange(3), np.arange(3)] = 0.0
        m[np.arange(3), np.arange(3)] = np.abs(m).sum(axis=1) + 1.0
        for i in range(3):
            for j in range(3):
                rows.append(3 * b + i), cols.append(3 * b + j), vals.append(m[i, j])
    return csr_from_coo(3 * blocks, rows, cols, vals)


def transposed_positions(n, rp, ci):
    """for every stored position p = (i,j) the position of (j,i) (the pattern is structurally symmetric)"""
    where = [{int(ci[q]): q for q in range(rp[k], rp[k + 1])} for k in range(n)]
    return np.array([where[int(ci[p])][i] for i in range(n) for p in range(rp[i], rp[i + 1])], np.int64)
