"""Shared helpers of tests/test_amg_host.py, tests/test_gpu_amg.py and tests/test_gpu_cg_amg.py: numpy restatements of
include/spmv/amg.h (the aggregation, the hierarchy, the V-cycle in fp32 and in fp64) and an exact prover of the
V-cycle in Fractions.  A plain module, not a conftest."""
from fractions import Fraction

import numpy as np

DENSE_ROWS = 1024


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def rows_of(n, rp):
    return np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))


def diag32(n, rp, ci, va):
    """fp32 sum of the stored (i,i) entries in storage order (0 where a row has none)"""
    d = np.zeros(n, np.float32)
    rows = rows_of(n, rp)
    where = np.flatnonzero(np.asarray(ci) == rows)
    owner = rows[where]                                         # ascending: a row's stored diagonals lie together
    nth = np.arange(where.size) - np.searchsorted(owner, owner)
    for k in range(int(nth.max(initial=-1)) + 1):               # the k-th stored diagonal of every row that has one
        pick = nth == k
        d[owner[pick]] = d[owner[pick]] + np.asarray(va, np.float32)[where[pick]]
    return d


def tridiagonal(n):
    """tridiag(-1, 2, -1), columns ascending"""
    rows, cols, vals = [], [], []
    for i in range(n):
        for j, v in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                rows.append(i), cols.append(j), vals.append(v)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def pair_maps(n, coarsest):
    """the maps {2a, 2a+1} -> a from n rows down to `coarsest` rows"""
    maps = []
    while n > coarsest:
        assert n % 2 == 0
        maps.append((np.arange(n) // 2).astype(np.int32))
        n //= 2
    assert n == coarsest
    return maps


# ---- aggregation ---------------------------------------------------------------------------------------------
def aggregate(n, rp, ci, va, theta):
    """amg.h's three passes, restated; (aggregate int32[n], count)"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    va = np.asarray(va, np.float32)
    d = diag32(n, rp, ci, va).astype(np.float64)
    rows = rows_of(n, rp)
    th = np.float64(np.float32(theta))
    v64 = va.astype(np.float64)
    with np.errstate(all="ignore"):
        strong = (ci != rows) & (va != 0) & (v64 * v64 >= (th * th) * np.abs(d[rows] * d[ci]))
    agg = np.full(n, -1, np.int64)
    count = 0
    neighbours = [ci[rp[i]:rp[i + 1]][strong[rp[i]:rp[i + 1]]] for i in range(n)]
    for i in range(n):
        if agg[i] != -1 or (agg[neighbours[i]] != -1).any():
            continue
        agg[i] = count
        agg[neighbours[i]] = count
        count += 1
    first = agg.copy()
    for i in range(n):
        if first[i] != -1:
            continue
        best, best_abs = -1, np.float32(0)
        for p in range(rp[i], rp[i + 1]):
            if strong[p] and first[ci[p]] != -1 and (best == -1 or abs(va[p]) > best_abs):
                best, best_abs = ci[p], abs(va[p])
        if best != -1:
            agg[i] = first[best]
    for i in range(n):
        if agg[i] != -1:
            continue
        agg[i] = count
        for j in neighbours[i]:
            if agg[j] == -1:
                agg[j] = count
        count += 1
    return agg.astype(np.int32), count


# ---- hierarchy -----------------------------------------------------------------------------------------------
def prolongation(n, agg):
    return np.arange(n + 1, dtype=np.int32), np.asarray(agg, np.int32), np.ones(n, np.float32)


def restriction(n, agg, count):
    """P^T as CSR: the members of each aggregate, rows ascending"""
    agg = np.asarray(agg, np.int64)
    order = np.argsort(agg, kind="stable")
    rp = np.zeros(count + 1, np.int32)
    np.cumsum(np.bincount(agg, minlength=count), out=rp[1:])
    return rp, order.astype(np.int32), np.ones(n, np.float32)


def galerkin(spmv, n, rp, ci, va, agg, count):
    """P^T (A P) by two spgemm_cpu_csr calls on the host: (row_ptrs, cols, vals) of the count x count matrix"""
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    P = spmv.csr_from_arrays(n, count, *prolongation(n, agg))
    PT = spmv.csr_from_arrays(count, n, *restriction(n, agg, count))
    AP, C = spmv.csr_create(0, 0, 0), spmv.csr_create(0, 0, 0)
    try:
        assert spmv.spgemm_cpu_csr(AP, A, P) == 0 and spmv.spgemm_cpu_csr(C, PT, AP) == 0
        assert (C.contents.num_rows, C.contents.num_cols) == (count, count)
        return spmv.csr_host_arrays(C)
    finally:
        for M in (A, P, PT, AP, C):
            spmv.csr_destroy(M)


def hierarchy(spmv, n, rp, ci, va, theta=0.08, coarse_rows=64, max_levels=10, maps=None):
    """The levels amg_setup builds, restated: a list of dicts n, rp, ci, va, agg (None on the coarsest), count."""
    levels = []
    while True:
        level = dict(n=n, rp=np.asarray(rp, np.int32), ci=np.asarray(ci, np.int32), va=np.asarray(va, np.float32),
                     agg=None, count=0)
        levels.append(level)
        l = len(levels) - 1
        if maps is not None:
            if l == min(len(maps), max_levels - 1):
                return levels
            agg = np.asarray(maps[l], np.int32)
            count = int(agg.max()) + 1
        else:
            if n <= coarse_rows or l + 1 == max_levels:
                return levels
            agg, count = aggregate(n, rp, ci, va, theta)
            if count == n:
                return levels
        level["agg"], level["count"] = agg, count
        rp, ci, va = galerkin(spmv, n, rp, ci, va, agg, count)
        n = count


def dense_of(level, dtype=np.float64):
    n = level["n"]
    out = np.zeros((n, n), dtype)
    np.add.at(out, (rows_of(n, level["rp"]), level["ci"]), level["va"].astype(dtype))
    return out


# ---- the V-cycle in numpy -------------------------------------------------------------------------------------
def _spmv(level, x, dtype):
    rp = np.asarray(level["rp"], np.int64)
    prod = level["va"].astype(dtype) * x[level["ci"]]
    out = np.zeros(level["n"], dtype)
    nonempty = rp[1:] > rp[:-1]
    if prod.size and nonempty.any():
        out[nonempty] = np.add.reduceat(prod, rp[:-1][nonempty])
    return out


def vcycle(levels, r, omega=2.0 / 3.0, pre=1, post=1, coarse_sweeps=4, dtype=np.float64, l=0):
    """One V-cycle of amg.h from a zero guess, every operation in `dtype` (row sums by np.add.reduceat, another order
    than the device's).  In fp32 wd and the dense inverse are the fp32 arrays the library stores; in fp64 they are not
    rounded."""
    level = levels[l]
    n = level["n"]
    f = np.asarray(r, dtype)
    w = np.float64(np.float32(omega))
    wd = w / diag32(n, level["rp"], level["ci"], level["va"]).astype(np.float64)
    wd = wd.astype(np.float32).astype(dtype) if dtype == np.float32 else wd

    def sweeps(count):
        x = (wd * f).astype(dtype)
        for _ in range(count - 1):
            x = (x + wd * (f - _spmv(level, x, dtype))).astype(dtype)
        return x

    if l == len(levels) - 1:
        if n > DENSE_ROWS:
            return sweeps(coarse_sweeps)
        dense = dense_of(level)
        if dtype == np.float32:
            inverse = np.linalg.inv(dense)
            return (((inverse + inverse.T) / 2).astype(np.float32) @ f).astype(np.float32)
        return np.linalg.solve(dense, f)
    x = sweeps(pre)
    res = (f - _spmv(level, x, dtype)).astype(dtype)
    fc = np.zeros(level["count"], dtype)
    np.add.at(fc, level["agg"], res)
    e = vcycle(levels, fc, omega, pre, post, coarse_sweeps, dtype, l + 1)
    x = (x + e[level["agg"]]).astype(dtype)
    for _ in range(post):
        x = (x + wd * (f - _spmv(level, x, dtype))).astype(dtype)
    return x


def tolerance(z32, z64):
    """The bound of the by-bound tests: 8 x the distance between the two restatements, at least 1e-6 ||z||_inf."""
    z64 = np.asarray(z64, np.float64)
    return max(8.0 * float(np.max(np.abs(np.asarray(z32, np.float64) - z64))), 1e-6 * float(np.max(np.abs(z64))))


# ---- the exact prover ------------------------------------------------------------------------------------------
class NotExact(Exception):
    pass


class Prover:
    """The V-cycle on tridiag(-1, 2, -1) with pair aggregates in Fractions.  Every sum the device forms, in whatever
    order its lanes take, has terms that are multiples of one power-of-two quantum q; when sum |terms| < 2^24 q every
    partial sum of every order is a multiple of q below 2^24 q, hence an fp32 number, and nothing rounds
    (exact_data.py's rule).  `bits` is the largest such sum met, in bits."""

    def __init__(self):
        self.bits = 0

    def total(self, terms):
        terms = [Fraction(t) for t in terms]
        scale = 1
        for t in terms:
            den = t.denominator
            if den & (den - 1):
                raise NotExact("not dyadic")
            scale = max(scale, den)
        units = sum(abs(t) * scale for t in terms)
        assert units.denominator == 1
        self.bits = max(self.bits, int(units).bit_length())
        if int(units) >= 1 << 24:
            raise NotExact("a sum needs %d bits" % int(units).bit_length())
        return sum(terms)

    def residual(self, n, f, x, i):
        terms = [f[i], -2 * x[i]]
        if i > 0:
            terms.append(x[i - 1])
        if i + 1 < n:
            terms.append(x[i + 1])
        return self.total(terms)

    def sweep(self, n, wd, f, x):
        return [self.total([wd * self.residual(n, f, x, i), x[i]]) for i in range(n)]

    def cycle(self, n, coarsest, f, omega, sweeps):
        if n == coarsest:               # inverse of tridiag(-1, 2, -1): (min(i,j) + 1) (n - max(i,j)) / (n + 1)
            inv = [[Fraction((min(i, j) + 1) * (n - max(i, j)), n + 1) for j in range(n)] for i in range(n)]
            for row in inv:
                for v in row:
                    self.total([v])     # the stored fp32 inverse is the exact one
            return [self.total([inv[i][j] * f[j] for j in range(n)]) for i in range(n)]
        wd = Fraction(omega) / 2
        x = [self.total([wd * f[i]]) for i in range(n)]
        for _ in range(sweeps - 1):
            x = self.sweep(n, wd, f, x)
        fc = [self.total([self.residual(n, f, x, 2 * a), self.residual(n, f, x, 2 * a + 1)]) for a in range(n // 2)]
        e = self.cycle(n // 2, coarsest, fc, omega, sweeps)
        x = [self.total([x[i], e[i // 2]]) for i in range(n)]
        for _ in range(sweeps):
            x = self.sweep(n, wd, f, x)
        return x


def prove_vcycle(n, coarsest, r, omega=0.5, sweeps=1):
    """(z as float32, bits) when every intermediate of the cycle is exact in fp32, else (None, reason)"""
    prover = Prover()
    try:
        z = prover.cycle(n, coarsest, [Fraction(int(v)) for v in r], Fraction(omega), sweeps)
    except NotExact as why:
        return None, str(why)
    out = np.array([float(v) for v in z], np.float32)
    assert all(Fraction(float(a)) == b for a, b in zip(out, z))
    return out, prover.bits


def exact_rhs(n, seed=5):
    return np.random.default_rng(seed).integers(-8, 9, n).astype(np.float32)
