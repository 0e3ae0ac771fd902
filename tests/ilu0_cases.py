"""Matrices and restatements shared by the ILU(0) tests (test_ilu0_host.py, test_gpu_ilu0.py, test_gpu_bicgstab_lu.py).

* numpy_ilu0: the arithmetic of include/spmv/ilu0.h restated entry by entry, the fma taken as the fp64 product and
  difference rounded once to fp32 (exact: the product of two fp32 values fits fp64, and where the fp64 sum is itself
  rounded the tests' values are far from a double-rounding tie; the exact cases below do not round at all).
* exact_tridiagonal / arrow: integer (dyadic) matrices whose pattern holds all the fill, so ILU(0) is the exact LU;
  prove_exact runs the recurrence in int64 fixed point, checks that every quotient and update is exact and
  representable in fp32, and that L U == A entry for entry, and returns the factor's values.
* sorted_random / block3: inexact shapes for the device tests.
"""
import numpy as np


def rows_of(n, rp):
    return np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))


def csr_from_coo(n, rows, cols, vals):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return n, rp, cols[order].astype(np.int32), np.asarray(vals, np.float32)[order]


def fma32(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def numpy_ilu0(n, rp, ci, va):
    """(lu_values, zero_pivot) by the rule of ilu0.h; rows strictly ascending with a stored diagonal"""
    lu = np.asarray(va, np.float32).copy()
    diag = np.full(n, -1, np.int64)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                diag[i] = j
    assert (diag >= 0).all()
    with np.errstate(all="ignore"):
        for i in range(n):
            for pk in range(rp[i], diag[i]):
                k = ci[pk]
                l = np.float32(lu[pk] / lu[diag[k]])
                lu[pk] = l
                where = {int(ci[q]): q for q in range(diag[k] + 1, rp[k + 1])}
                for t in range(pk + 1, rp[i + 1]):
                    q = where.get(int(ci[t]))
                    if q is not None:
                        lu[t] = fma32(-l, lu[q], lu[t])
    d = lu[diag]
    bad = np.flatnonzero(~((d != 0) & np.isfinite(d)))
    return lu, (int(bad[0]) if bad.size else -1)


def prove_exact(n, rp, ci, va, shift=0):
    """ILU(0) of (n, rp, ci, va) in int64 fixed point with `shift` fractional bits.  Asserts that A's values are
    multiples of 2^-shift, that every quotient and every update is exact and below 2^24 units (so fp32 holds it and
    no operation rounds), and that L U == A on and off the pattern (ILU(0) is the exact LU).  Returns the factor."""
    one = 1 << shift
    a = np.asarray(va, np.float64) * one
    w = np.rint(a).astype(np.int64)
    assert (w == a).all()
    w = [int(v) for v in w]
    diag = {}
    for i in range(n):
        cols = ci[rp[i]:rp[i + 1]]
        assert (np.diff(cols) > 0).all()
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                diag[i] = j
    assert len(diag) == n
    limit = 1 << 24
    for i in range(n):
        for pk in range(rp[i], diag[i]):
            k = int(ci[pk])
            num = w[pk] * one
            assert w[diag[k]] != 0 and num % w[diag[k]] == 0
            l = num // w[diag[k]]
            assert abs(l) < limit
            w[pk] = l
            where = {int(ci[q]): q for q in range(diag[k] + 1, rp[k + 1])}
            for t in range(pk + 1, rp[i + 1]):
                q = where.get(int(ci[t]))
                if q is not None:
                    prod = l * w[q]
                    assert prod % one == 0
                    w[t] -= prod // one
                    assert abs(w[t]) < limit
    # L U == A, and nothing outside the pattern
    for i in range(n):
        acc = {}
        terms = [(int(ci[p]), w[p]) for p in range(rp[i], diag[i])] + [(i, one)]
        for k, l in terms:
            for q in range(diag[k], rp[k + 1]):
                acc[int(ci[q])] = acc.get(int(ci[q]), 0) + l * w[q]
        want = {int(ci[p]): int(round(float(va[p]) * one)) * one for p in range(rp[i], rp[i + 1])}
        for j, v in acc.items():
            assert v == want.get(j, 0), (i, j)
        for j, v in want.items():
            assert acc.get(j, 0) == v, (i, j)
    lu = (np.array(w, np.float64) / one).astype(np.float32)
    assert (lu.astype(np.float64) * one == np.array(w, np.float64)).all()
    return lu


def exact_tridiagonal(n, lower=-1, diag=4, upper=-2, seed=None):
    """A = L U, L unit lower bidiagonal (sub-diagonal `lower`), U upper bidiagonal (`diag`, `upper`), small integers
    (constant, or drawn per row with `seed`).  Returns (n, rp, ci, va, lu) with lu the factor in A's pattern."""
    if seed is None:
        l = np.full(n, lower, np.int64)
        d = np.full(n, diag, np.int64)
        u = np.full(n, upper, np.int64)
    else:
        rng = np.random.default_rng(seed)
        l = rng.choice([-3, -2, -1, 1, 2, 3], n)
        d = rng.choice([2, 3, 4, 5, -4], n)
        u = rng.choice([-3, -2, -1, 1, 2, 3], n)
    rows, cols, vals, fact = [], [], [], []
    for i in range(n):
        if i > 0:
            rows.append(i), cols.append(i - 1), vals.append(l[i] * d[i - 1]), fact.append(l[i])
        rows.append(i), cols.append(i), vals.append(d[i] + (l[i] * u[i - 1] if i > 0 else 0)), fact.append(d[i])
        if i + 1 < n:
            rows.append(i), cols.append(i + 1), vals.append(u[i]), fact.append(u[i])
    n, rp, ci, va = csr_from_coo(n, rows, cols, vals)          # (already in order)
    return n, rp, ci, va, np.array(fact, np.float32)


def arrow(n, seed=7):
    """power-of-two diagonal, integer last row and last column, the corner large enough to stay non-zero; the only fill
    lands on the stored corner.  Values are multiples of 1/8 after the factorisation: prove with shift=3."""
    rng = np.random.default_rng(seed)
    d = rng.choice([1, 2, 4, 8], n - 1)
    right = rng.integers(-4, 5, n - 1)
    bottom = rng.integers(-4, 5, n - 1)
    right[right == 0] = 1
    bottom[bottom == 0] = -1
    rows, cols, vals = [], [], []
    for i in range(n - 1):
        rows += [i, i]
        cols += [i, n - 1]
        vals += [d[i], right[i]]
    rows += [n - 1] * n
    cols += list(range(n))
    vals += list(bottom) + [64 * n]
    return csr_from_coo(n, rows, cols, vals)


def sorted_random(n, per_row, seed):
    """strictly row diagonally dominant, non-symmetric, about per_row stored entries per row, columns de-duplicated
    and ascending"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for i in range(n):
        c = np.unique(rng.integers(0, n, per_row - 1))
        c = c[c != i]
        v = rng.uniform(-1.0, 1.0, c.size)
        rows += [i] * (c.size + 1)
        cols += list(c) + [i]
        vals += list(v) + [np.abs(v).sum() + 1.0]
    return csr_from_coo(n, rows, cols, vals)


def block3(blocks, seed=5):
    """`blocks` independent dense 3 x 3 diagonally dominant blocks: three levels, each `blocks` rows wide"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for b in range(blocks):
        m = rng.uniform(-1.0, 1.0, (3, 3))
        m[np.arange(3), np.arange(3)] = np.abs(m).sum(axis=1) + 1.0
        for i in range(3):
            for j in range(3):
                rows.append(3 * b + i), cols.append(3 * b + j), vals.append(m[i, j])
    return csr_from_coo(3 * blocks, rows, cols, vals)
