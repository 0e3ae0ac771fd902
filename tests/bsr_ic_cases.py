"""Cases of block IC(0), the block triangular solves and cg_solve_bsr_ic (include/spmv/bsr_factor.h, include/spmv/cg.h,
DESIGN.md §4.31), shared by tests/test_bsr_ic_host.py (no GPU) and tests/test_gpu_bsr_ic.py.

Restatements.  ic0() is bsr_factor.h's definition written once over an arithmetic `ops`: Float32Ops rounds like the
library (fma32 of ilu0_cases.py for the fused steps, Python floats, which are IEEE doubles rounded per operation, for
the diagonal stage); ExactOps runs the same program in rationals and asserts that EVERY intermediate is a float32
(stages 1 - 3) or a double (the diagonal stage), which proves that the rounded program makes no rounding error at all on
that input.  solve() is sptrsv_cpu_bsr's rule in numpy float32; restate_cg() with ic_apply() is cg.h's iteration with it.

The exact family: block patterns on which IC(0) is the complete Cholesky factorisation (no fill): forests of F chains
of length l (block tridiagonal; F = 1 is a chain, l = 1 is block diagonal) and an arrow with the hub last.  A = L L^T
is formed in int64 from a chosen L whose diagonal blocks are lower triangular with diagonal entries in {1, 2} and
small integers below, and whose off-diagonal blocks hold {-1, 0, 1, 2}; b = 8 takes sparser blocks.  Ragged sizes cut
the last block row and column.

The float family: weighted graph Laplacians of §4.29's block structures (2-D 9-point, 3-D 7-point, 3-D 27-point, and
one with 45 % of the off-diagonal positions dropped, symmetrically, so that IC(0) really drops fill) (x) K + 0.05 I with
K[i][j] = min(i, j) + 1: SPD, weakly dominant, strongly coupled inside a node; and block_spd of cg_bsr_cases.py, full
strongly coupled blocks on a random SPD node pattern: irregular, with block rows of different lengths."""
import math
from fractions import Fraction

import numpy as np

import cg_bsr_cases as cc
from ilu0_cases import fma32

BLOCK_DIMS = (2, 3, 4, 8)
LANES = (1, 2, 4, 8, 16, 32, 64)
K_BLOCK = 256                      # kBlock (csrc/device_common.h)
ROW_BLOCKS = 2048                  # kMaxResidentBlocks: the grid cap of a wide level
NARROW = 256                       # kSptrsvNarrowRows (csrc/internal.h)
MAX_RUN_LEVELS = 8192              # kSptrsvMaxRunLevels
LOWER, UPPER = 0, 1


def forced(monkeypatch, lanes, more=""):
    monkeypatch.setenv("SPMV_DEBUG", "bsr_tri_lanes=%d%s" % (lanes, more))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what=""):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


# ------------------------------------------------------------------------------------------ arithmetic
def is_float(q, mant, emin):
    """the rational q is a binary float with `mant` significand bits and least exponent emin (of the last place)"""
    if q == 0:
        return True
    num, den = abs(q.numerator), q.denominator
    if den & (den - 1):
        return False
    shift = den.bit_length() - 1                   # q = num / 2^shift
    low = (num & -num).bit_length() - 1             # trailing zeros of num
    return num.bit_length() - low <= mant and low - shift >= emin


class Float32Ops:
    """the library's roundings"""
    zero = np.float32(0.0)

    @staticmethod
    def load(v):
        return np.float32(v)

    @staticmethod
    def fma(a, b, c):
        return fma32(a, b, c)

    @staticmethod
    def neg(a):
        return np.float32(-a)

    # the diagonal stage: Python floats are doubles, every operation rounded on its own
    @staticmethod
    def wide(v):
        return float(v)

    @staticmethod
    def sqrt(w):
        return math.sqrt(w) if w >= 0.0 else float("nan")

    @staticmethod
    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    @staticmethod
    def narrow(w):
        with np.errstate(all="ignore"):
            return np.float32(w)

    @staticmethod
    def good(w):
        return w > 0.0 and math.isfinite(w)


class ExactOps:
    """the same program in rationals; every intermediate must be representable"""
    zero = Fraction(0)
    count = 0

    @classmethod
    def _f32(cls, q):
        cls.count += 1
        assert is_float(q, 24, -149), ("not a float32", q)
        return q

    @classmethod
    def _f64(cls, q):
        cls.count += 1
        assert is_float(q, 53, -1074), ("not a double", q)
        return q

    @classmethod
    def load(cls, v):
        return cls._f32(Fraction(float(v)))

    @classmethod
    def fma(cls, a, b, c):
        return cls._f32(a * b + c)

    @staticmethod
    def neg(a):
        return -a

    @classmethod
    def wide(cls, v):
        return _Wide(v)

    @classmethod
    def sqrt(cls, w):
        q = w.q
        rn, rd = math.isqrt(q.numerator), math.isqrt(q.denominator)
        assert rn * rn == q.numerator and rd * rd == q.denominator, ("not a perfect square", q)
        return _Wide(cls._f64(Fraction(rn, rd)))

    @classmethod
    def div(cls, a, b):
        return _Wide(cls._f64(_q(a) / _q(b)))

    @classmethod
    def narrow(cls, w):
        return cls._f32(_q(w))

    @staticmethod
    def good(w):
        return _q(w) > 0


def _q(v):
    return v.q if isinstance(v, _Wide) else Fraction(v)


class _Wide:
    """a double of the diagonal stage in the exact program: +, -, * check representability"""

    def __init__(self, q):
        self.q = _q(q)

    def __mul__(self, o):
        return _Wide(ExactOps._f64(self.q * _q(o)))

    __rmul__ = __mul__

    def __add__(self, o):
        return _Wide(ExactOps._f64(self.q + _q(o)))

    __radd__ = __add__

    def __sub__(self, o):
        return _Wide(ExactOps._f64(self.q - _q(o)))

    def __rsub__(self, o):
        return _Wide(ExactOps._f64(_q(o) - self.q))

    def __neg__(self):
        return _Wide(-self.q)

    def __gt__(self, o):
        return self.q > _q(o)


# ------------------------------------------------------------------------------------------ the factorisation
def diagonal_positions(brp, bc):
    nb = len(brp) - 1
    diag = np.full(nb, -1, np.int64)
    for I in range(nb):
        for p in range(brp[I], brp[I + 1]):
            if bc[p] == I:
                diag[I] = p
    assert (diag >= 0).all()
    return diag


def ic0(n, b, brp, bc, bv, ops=Float32Ops):
    """(f [num_blocks][b][b] nested lists of ops' numbers, bad_pivot) by bsr_factor.h's rule; block columns strictly
    ascending, every diagonal block stored, a structurally symmetric block pattern"""
    nb = len(brp) - 1
    bv = np.asarray(bv, np.float32).reshape(-1, b, b)
    diag = diagonal_positions(brp, bc)
    f = [None] * len(bc)
    nxt = [int(d) + 1 for d in diag]
    bad = -1
    rng = range(b)
    for I in range(nb):
        size = min(b, n - I * b)
        di = int(diag[I])
        for t in range(brp[I], di + 1):
            f[t] = [[ops.load(bv[t, r, c]) for c in rng] for r in rng]
        W = f[di]
        for pk in range(brp[I], di):
            K = int(bc[pk])
            V = f[int(diag[K])]
            w = f[pk]
            L = [[ops.zero] * b for _ in rng]
            for r in range(size):
                for c in rng:
                    s = ops.zero
                    for m in range(c + 1):
                        s = ops.fma(w[r][m], V[c][m], s)
                    L[r][c] = s
            f[pk] = L
            cols_k = {int(bc[q]): q for q in range(int(diag[K]) + 1, brp[K + 1])}
            for t in range(pk + 1, di):
                q = cols_k.get(int(bc[t]))
                if q is None:
                    continue
                Fq, Wt = f[q], f[t]
                for r in range(size):
                    for c in rng:
                        s = Wt[r][c]
                        for m in rng:
                            s = ops.fma(ops.neg(L[r][m]), Fq[m][c], s)
                        Wt[r][c] = s
            for r in range(size):
                for c in range(r + 1):
                    s = W[r][c]
                    for m in rng:
                        s = ops.fma(ops.neg(L[r][m]), L[c][m], s)
                    W[r][c] = s
            up = nxt[K]
            nxt[K] += 1
            assert bc[up] == I
            f[up] = [[L[r][m] for r in rng] for m in rng]
        # the diagonal stage in doubles: Cholesky row by row, then the inverse of the factor column by column
        T = [[ops.wide(W[r][c]) if r < size else None for c in range(r + 1)] for r in rng]
        ok = True
        for p in range(size):
            for q in range(p + 1):
                w = T[p][q]
                for k in range(q):
                    w = w - T[p][k] * T[q][k]
                if q == p:
                    ok = ok and ops.good(w)
                    T[p][p] = ops.sqrt(w)
                else:
                    T[p][q] = ops.div(w, T[q][q])
        for j in range(size):
            T[j][j] = ops.div(1.0 if ops is Float32Ops else Fraction(1), T[j][j])
            for i in range(j + 1, size):
                t = ops.wide(0.0)
                for k in range(j, i):
                    t = t + T[i][k] * T[k][j]
                T[i][j] = ops.div(-t, T[i][i])
        if not ok and bad < 0:
            bad = I
        Vd = [[ops.zero] * b for _ in rng]
        for r in range(size):
            for c in range(r + 1):
                Vd[r][c] = Vd[c][r] = ops.narrow(T[r][c])
        f[di] = Vd
    return f, bad


def factor_array(f, b):
    """the nested factor as the flat float32 array the library stores"""
    with np.errstate(all="ignore"):
        return np.array([[[float(_q(x)) if not isinstance(x, np.floating) else x for x in row] for row in blk]
                         for blk in f], np.float32).reshape(-1)


# ------------------------------------------------------------------------------------------ the solve
def solve(n, b, brp, bc, fv, rhs, uplo, unit=False):
    """sptrsv_cpu_bsr's rule in numpy float32"""
    nb = len(brp) - 1
    F = np.asarray(fv, np.float32).reshape(-1, b, b)
    rhs = np.asarray(rhs, np.float32)
    x = np.zeros(nb * b, np.float32)
    with np.errstate(all="ignore"):
        for I in (range(nb - 1, -1, -1) if uplo == UPPER else range(nb)):
            size = min(b, n - I * b)
            s = np.zeros(b, np.float32)
            d = -1
            for p in range(brp[I], brp[I + 1]):
                J = int(bc[p])
                if J == I:
                    d = p
                if (J <= I) if uplo == UPPER else (J >= I):
                    continue
                for c in range(min(b, n - J * b)):
                    s = (s + (F[p][:, c] * x[J * b + c]).astype(np.float32)).astype(np.float32)
            t = np.zeros(b, np.float32)
            t[:size] = (rhs[I * b:I * b + size] - s[:size]).astype(np.float32)
            if unit:
                x[I * b:I * b + size] = t[:size]
                continue
            for r in range(size):
                u = np.float32(0.0)
                for c in (range(r, size) if uplo == UPPER else range(r + 1)):
                    u = np.float32(u + np.float32(F[d][r, c] * t[c]))
                x[I * b + r] = u
    return x[:n]


# ------------------------------------------------------------------------------------------ products and CG
def expand(n, b, brp, bc, bv):
    """dense float64 n x n matrix of the BSR arrays"""
    nb = len(brp) - 1
    M = np.zeros((nb * b, nb * b))
    blocks = np.asarray(bv, np.float64).reshape(-1, b, b)
    for I in range(nb):
        for p in range(brp[I], brp[I + 1]):
            J = int(bc[p])
            M[I * b:(I + 1) * b, J * b:(J + 1) * b] = blocks[p]
    return M[:n, :n]


def restate_cg(A64, rhs, tol, apply, max_iter=2000, spmv=None):
    """cg.h's iteration in numpy (cg_bsr_cases.restate's rules) with z = apply(r); A64 dense float64 holding the float32
    entries; returns (x, iterations, converged, breakdown, relative residual).  spmv(v): another correct realisation
    of q = A p (other_products) in place of the product rounded from fp64 sums."""
    rhs = np.asarray(rhs, np.float32)
    n = rhs.size
    x = np.zeros(n, np.float32)
    if spmv is None:
        spmv32 = lambda v: (A64 @ v.astype(np.float64)).astype(np.float32)
    else:
        spmv32 = lambda v: np.asarray(spmv(v)).astype(np.float32)
    dot = lambda a, c: float(np.dot(a.astype(np.float64), c.astype(np.float64)))
    r = rhs.copy()
    z = apply(r)
    p = z.copy()
    rz, rr, bb = dot(r, z), dot(r, r), dot(rhs, rhs)
    bnorm = np.sqrt(bb)
    thr = float(np.float32(tol)) * bnorm
    it, conv, brk, rel = 0, False, False, np.sqrt(rr) / bnorm
    if not rz > 0:
        return x, 0, False, True, rel
    for k in range(max_iter):
        q = spmv32(p)
        pq = dot(p, q)
        if not pq > 0:
            brk = True
            break
        a = np.float64(np.float32(rz / pq))
        x = (a * p.astype(np.float64) + x).astype(np.float32)
        r = (-a * q.astype(np.float64) + r).astype(np.float32)
        z = apply(r)
        rz_new, rr = dot(r, z), dot(r, r)
        it, rel = k + 1, np.sqrt(rr) / bnorm
        if np.sqrt(rr) <= thr:
            conv = True
            break
        if not rz_new > 0:
            brk = True
            break
        beta = np.float64(np.float32(rz_new / rz))
        p = (beta * p.astype(np.float64) + z).astype(np.float32)
        rz = rz_new
    return x, it, conv, brk, rel


def other_products(n, b, brp, bc, bv):
    """the five other realisations of q = A p that cg_bsr_cases.reference_spread compares, as functions of p: the
    product summed in fp32, three with roundoff-sized noise, and the product in the lane-group kernel's documented
    order, all on the CSR expansion of the BSR arrays (every position of every block, as spmv_bsr multiplies them)"""
    rp, ci, va = cc.bsr_to_csr_arrays(n, b, brp, bc, bv)
    products = [cc.spmv_fp32, cc.spmv_noisy(1), cc.spmv_noisy(2), cc.spmv_noisy(3), cc.spmv_lane_order(n, b, rp, ci, va)]
    return [lambda v, f=f: f(rp, ci, va, v) for f in products]


def ic_apply(n, b, brp, bc, fv):
    return lambda r: solve(n, b, brp, bc, fv, solve(n, b, brp, bc, fv, r, LOWER), UPPER)


def block_jacobi_apply(n, b, brp, bc, bv):
    """z = D^-1 r with the fp64 inverses of the diagonal blocks rounded to float32 (the steps compared are far apart)"""
    nb = len(brp) - 1
    diag = diagonal_positions(brp, bc)
    blocks = np.asarray(bv, np.float64).reshape(-1, b, b)[diag]
    inv = np.zeros((nb, b, b), np.float32)
    for I in range(nb):
        size = min(b, n - I * b)
        inv[I, :size, :size] = np.linalg.inv(blocks[I, :size, :size]).astype(np.float32)

    def apply(r):
        rp = np.zeros(nb * b, np.float32)
        rp[:n] = r
        return np.einsum("ikc,ic->ik", inv.astype(np.float64), rp.reshape(nb, b).astype(np.float64)).astype(
            np.float32).ravel()[:n]
    return apply


# ------------------------------------------------------------------------------------------ the float family
def k_block(b):
    i = np.arange(b)
    return (np.minimum(i[:, None], i[None, :]) + 1).astype(np.float64)


def grid_pattern(kind, m, drop=0.0, seed=0):
    """sorted (rows, cols) of the off-diagonal neighbours of a grid graph: '2d9' (m x m, 9-point), '3d7', '3d27'
    (m x m x m); `drop` of the undirected edges removed"""
    dim = 2 if kind == "2d9" else 3
    idx = np.arange(m ** dim).reshape((m,) * dim)
    offs = []
    for o in np.ndindex((3,) * dim):
        o = tuple(v - 1 for v in o)
        if not any(o) or (kind == "3d7" and sum(abs(v) for v in o) != 1):
            continue
        offs.append(o)
    pairs = set()
    for o in offs:
        src = tuple(slice(max(0, -v), m - max(0, v)) for v in o)
        dst = tuple(slice(max(0, v), m - max(0, -v)) for v in o)
        for a, c in zip(idx[src].ravel(), idx[dst].ravel()):
            pairs.add((min(int(a), int(c)), max(int(a), int(c))))
    pairs = sorted(pairs)
    if drop > 0.0:
        keep = np.random.default_rng(seed).uniform(size=len(pairs)) >= drop
        pairs = [p for p, k in zip(pairs, keep) if k]
    return m ** dim, pairs


def laplacian_bsr(nodes, pairs, b, n=None, seed=1, weights=True, shift=0.05):
    """(n, brp, bc, bv): (weighted graph Laplacian of `pairs`) (x) K + shift I as BSR arrays, block columns ascending;
    n < nodes * b cuts the last block row and column (the positions outside hold +0.0f)"""
    n = nodes * b if n is None else n
    assert (nodes - 1) * b < n <= nodes * b
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 1.5, len(pairs)) if weights else np.ones(len(pairs))
    entries = {}
    deg = np.zeros(nodes)
    for (i, j), wij in zip(pairs, w):
        entries[(i, j)] = entries[(j, i)] = -wij
        deg[i] += wij
        deg[j] += wij
    for i in range(nodes):
        entries[(i, i)] = deg[i]
    keys = sorted(entries)
    brp = np.zeros(nodes + 1, np.int32)
    for i, _ in keys:
        brp[i + 1] += 1
    brp = np.cumsum(brp).astype(np.int32)
    bc = np.array([j for _, j in keys], np.int32)
    K = k_block(b)
    bv = np.zeros((len(keys), b, b))
    for p, (i, j) in enumerate(keys):
        bv[p] = entries[(i, j)] * K + (shift * np.eye(b) if i == j else 0.0)
        for side, node in ((0, i), (1, j)):
            inside = min(b, n - node * b)
            if inside < b:
                if side == 0:
                    bv[p, inside:, :] = 0.0
                else:
                    bv[p, :, inside:] = 0.0
    return n, brp, bc, bv.astype(np.float32).reshape(-1)


def laplacian_system(m, b):
    """the issue's system: (2-D 5-point Laplacian on an m x m grid) (x) K + 0.05 I, unweighted"""
    idx = np.arange(m * m).reshape(m, m)
    pairs = [(int(a), int(c)) for a, c in zip(idx[:, :-1].ravel(), idx[:, 1:].ravel())]
    pairs += [(int(a), int(c)) for a, c in zip(idx[:-1, :].ravel(), idx[1:, :].ravel())]
    return laplacian_bsr(m * m, sorted(pairs), b, weights=False)


def float_family(b, small=True):
    """[(name, n, brp, bc, bv)]: the structures of the module docstring, full and ragged"""
    m2, m3 = (5, 3) if small else (24, 9)
    out = []
    for name, kind, m, drop in (("2d9", "2d9", m2, 0.0), ("3d7", "3d7", m3, 0.0), ("3d27", "3d27", m3, 0.0),
                                ("2d9-dropped", "2d9", m2 + 1, 0.45)):
        nodes, pairs = grid_pattern(kind, m, drop, seed=7)
        for cut in ((0,) if name == "3d27" else range(b) if name == "2d9" else (0, b - 1)):
            out.append(("%s b=%d cut=%d" % (name, b, cut),) + laplacian_bsr(nodes, pairs, b, nodes * b - cut, seed=b))
    nodes = 14 if small else 700
    for cut in (0, b - 1):
        out.append(("block_spd b=%d cut=%d" % (b, cut),) + block_spd_bsr(nodes * b - cut, b, seed=40 + b))
    return out


def csr_to_bsr(n, b, rp, ci, va):
    """(brp, bc, bv) of a CSR matrix with ascending columns: bsr_from_csr_cpu's rule in numpy (a block for every block
    column a block row touches, ascending; the positions A does not store hold +0.0f)"""
    nb = -(-n // b)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))
    cols = np.asarray(ci, np.int64)
    uniq, where = np.unique((rows // b) * nb + cols // b, return_inverse=True)
    bv = np.zeros((uniq.size, b, b), np.float32)
    bv[where, rows % b, cols % b] = va
    brp = np.concatenate([[0], np.cumsum(np.bincount(uniq // nb, minlength=nb))]).astype(np.int32)
    return brp, (uniq % nb).astype(np.int32), bv.reshape(-1)


def block_spd_bsr(n, b, seed, coupling=0.3):
    """(n, brp, bc, bv): block_spd of cg_bsr_cases.py, b unknowns per node on a random SPD node pattern with strongly
    coupled full blocks: an irregular symmetric block pattern with block rows of different lengths"""
    n, rp, ci, va = cc.block_spd(n, b, seed=seed, coupling=coupling)
    return (n,) + csr_to_bsr(n, b, rp, ci, va)


# (b, seed) of block_spd matrices of 300 b - 1 rows at coupling 0.9 on which IC(0) itself meets a pivot that is not > 0:
# A is SPD, the fill that IC(0) drops on the irregular pattern is what breaks it (found on the CPU with bsr_ic0_cpu)
BREAKDOWN_SPD = ((3, 5, 137), (8, 1, 279))                # (b, seed, bad_pivot)


PARITY_TOL = 1e-6
PARITY_SEEDS = {2: 1, 3: 4, 4: 3, 8: 1}                 # of the right-hand side of the Laplacian system
PARITY_SPD_SEEDS = {2: 1, 3: 1, 4: 1, 8: 1}             # of the block_spd matrix and its right-hand side


def parity_systems(b):
    """[(name, n, brp, bc, bv, rhs, tol)]: the float systems the device solver is held against the restatement on, chosen
    on the CPU alone by the two rules tests/test_bsr_ic_host.py asserts"""
    nodes, pairs = grid_pattern("2d9", 9 if b < 8 else 6)
    n, brp, bc, bv = laplacian_bsr(nodes, pairs, b, nodes * b - (b - 1), seed=b)
    rhs = np.random.default_rng([b, PARITY_SEEDS[b]]).uniform(-1.0, 1.0, n).astype(np.float32)
    out = [("2d9 b=%d" % b, n, brp, bc, bv, rhs, PARITY_TOL)]
    seed = PARITY_SPD_SEEDS[b]
    n, brp, bc, bv = block_spd_bsr((90 if b < 8 else 50) * b - (b - 1), b, seed)
    rhs = np.random.default_rng([b, seed, 7]).uniform(-1.0, 1.0, n).astype(np.float32)
    return out + [("block_spd b=%d" % b, n, brp, bc, bv, rhs, PARITY_TOL)]


# ------------------------------------------------------------------------------------------ the exact family
def _diag_block(b, k):
    """lower triangular, diagonal in {1, 2}, small integers below; sparser for b = 8"""
    D = np.zeros((b, b), np.int64)
    for r in range(b):
        D[r, r] = 1 + (r + k) % 2
        for c in range(r):
            if b < 8 or (r - c) == 1:
                D[r, c] = ((r * 3 + c + k) % 3) - 1
    return D


def _off_block(b, k):
    O = np.zeros((b, b), np.int64)
    for r in range(b):
        for c in range(b):
            if b < 8 or (r + c + k) % 4 == 0:
                O[r, c] = ((r * 5 + c * 3 + k) % 4) - 1          # {-1, 0, 1, 2}
    return O


def exact_forest(chains, length, b, n=None):
    """dict of a forest of `chains` chains of `length` block rows each, chain c holding the block rows c * length ..:
    A = L L^T in int64 (block tridiagonal inside a chain), as BSR arrays, with L's blocks and the exact V = L_II^-1.
    Built with array operations: the sizes go past the grid caps."""
    nb = chains * length
    n = nb * b if n is None else n
    assert (nb - 1) * b < n <= nb * b
    kinds = 4
    Dk = np.stack([_diag_block(b, k) for k in range(kinds)])
    Ok = np.stack([_off_block(b, k) for k in range(kinds)])
    I = np.arange(nb)
    dk = I % kinds
    has_left = I % length != 0
    ok = (I * 7 + 1) % kinds
    Ld = Dk[dk].copy()                                           # L_II
    Lo = np.where(has_left[:, None, None], Ok[ok], 0)            # L_{I,I-1}
    size = np.minimum(b, n - I * b)
    cut = np.arange(b)[None, :] >= size[:, None]                 # rows of the last block row outside the matrix
    Ld[cut] = 0
    Ld = np.where(cut[:, None, :], 0, Ld)
    Lo[cut] = 0
    Add = np.einsum("irm,icm->irc", Ld, Ld) + np.einsum("irm,icm->irc", Lo, Lo)
    Alo = np.einsum("irm,icm->irc", Lo[1:], Ld[:-1])             # A_{I,I-1} = L_{I,I-1} L_{I-1,I-1}^T
    has_right = np.concatenate([has_left[1:], [False]])
    counts = 1 + has_left.astype(np.int64) + has_right
    brp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nblocks = int(brp[-1])
    bc = np.zeros(nblocks, np.int32)
    av = np.zeros((nblocks, b, b), np.int64)
    lv = np.zeros((nblocks, b, b), np.int64)                     # the factor format with L_II in place of V
    pos_left = brp[:-1].astype(np.int64)
    pos_diag = pos_left + has_left
    pos_right = pos_diag + 1
    bc[pos_diag] = I
    av[pos_diag] = Add
    sel = np.flatnonzero(has_left)
    bc[pos_left[sel]] = sel - 1
    av[pos_left[sel]] = Alo[sel - 1]
    lv[pos_left[sel]] = Lo[sel]
    selr = np.flatnonzero(has_right)
    bc[pos_right[selr]] = selr + 1
    av[pos_right[selr]] = np.transpose(Alo[selr], (0, 2, 1))
    lv[pos_right[selr]] = np.transpose(Lo[selr + 1], (0, 2, 1))
    # V = L_II^-1: dyadic; one inverse per kind of diagonal block (the cut last block: its leading part)
    V = np.zeros((nb, b, b))
    for k in range(kinds):
        V[dk == k] = np.linalg.inv(Dk[k].astype(np.float64))
    if size[-1] < b:
        s = int(size[-1])
        V[-1] = 0.0
        V[-1, :s, :s] = np.linalg.inv(Dk[dk[-1]][:s, :s].astype(np.float64))
    Vsym = np.tril(V) + np.transpose(np.tril(V, -1), (0, 2, 1))
    fv = lv.astype(np.float32)
    fv[pos_diag] = Vsym.astype(np.float32)
    return dict(n=n, b=b, nb=nb, brp=brp, bc=bc, bv=av.astype(np.float32).reshape(-1), fv=fv.reshape(-1))


def exact_arrow(spokes, b, n=None):
    """an arrow with the hub last: block rows 0 .. spokes-1 are diagonal, the last block row is full"""
    nb = spokes + 1
    n = nb * b if n is None else n
    size_h = n - spokes * b
    assert 0 < size_h <= b
    Ld = [_diag_block(b, k) for k in range(nb)]
    Lh = [_off_block(b, k) for k in range(spokes)]
    Ld[-1][size_h:, :] = 0
    Ld[-1][:, size_h:] = 0
    for O in Lh:
        O[size_h:, :] = 0
    brp, bc, av, lv = [0], [], [], []
    for K in range(spokes):
        bc += [K, spokes]
        av += [Ld[K] @ Ld[K].T, (Lh[K] @ Ld[K].T).T]
        lv += [None, Lh[K].T]
        brp.append(len(bc))
    for K in range(spokes):
        bc.append(K)
        av.append(Lh[K] @ Ld[K].T)
        lv.append(Lh[K])
    bc.append(spokes)
    av.append(Ld[-1] @ Ld[-1].T + sum(O @ O.T for O in Lh))
    lv.append(None)
    brp.append(len(bc))
    fv = np.zeros((len(bc), b, b), np.float32)
    for p, blk in enumerate(lv):
        if blk is not None:
            fv[p] = blk
            continue
        I = bc[p]
        s = size_h if I == spokes else b
        Vi = np.zeros((b, b))
        Vi[:s, :s] = np.linalg.inv(Ld[I][:s, :s].astype(np.float64))
        fv[p] = np.tril(Vi) + np.tril(Vi, -1).T
    return dict(n=n, b=b, nb=nb, brp=np.array(brp, np.int32), bc=np.array(bc, np.int32),
                bv=np.array(av, np.float32).reshape(-1), fv=fv.reshape(-1))


def exact_solution(s, seed=3):
    """(x, rhs): a small integer x and rhs = A x in int64, as float32 (exact)"""
    n, b = s["n"], s["b"]
    x = np.random.default_rng(seed).integers(-3, 4, n).astype(np.int64)
    xp = np.zeros(s["nb"] * b, np.int64)
    xp[:n] = x
    blocks = np.asarray(s["bv"], np.float64).reshape(-1, b, b).astype(np.int64)
    rows = np.repeat(np.arange(s["nb"]), np.diff(s["brp"].astype(np.int64)))
    y = np.zeros((s["nb"], b), np.int64)
    np.add.at(y, rows, np.einsum("prc,pc->pr", blocks, xp.reshape(-1, b)[s["bc"]]))
    return x.astype(np.float32), y.ravel()[:n].astype(np.float32)


def solve_partial_sum_bound(s, x):
    """The largest value that sum |F||v| reaches in any row of either solve with the exact factor, for the integer
    solution x of A x = rhs, in units of the finest bit any term can carry.  LOWER solves L y = rhs: the off-diagonal sum
    of block row I is at most sum_{J<I} |L_IJ||y_J|, t = L_II y_I, and the diagonal step sums V_I t.  UPPER solves
    L^T x = y alike.  L's entries and x, y, rhs are integers; V's entries are dyadic with denominator at most
    2^(b-1) (diagonal entries 1 or 2), so every partial sum, in any order, is a multiple of 2^-(b-1) below the bound and
    a float32 when bound * 2^(b-1) < 2^24."""
    n, b, nb = s["n"], s["b"], s["nb"]
    full = expand(nb * b, b, s["brp"], s["bc"], s["fv"])
    strict = np.zeros_like(full)
    V = np.zeros_like(full)
    Ld = np.zeros_like(full)
    for I in range(nb):
        sl = slice(I * b, (I + 1) * b)
        strict[sl, :I * b] = full[sl, :I * b]
        size = min(b, n - I * b)
        V[sl, sl] = np.tril(full[sl, sl])
        Ld[I * b:I * b + size, I * b:I * b + size] = np.linalg.inv(V[sl, sl][:size, :size])
    L = strict + Ld
    xp = np.zeros(nb * b)
    xp[:n] = x
    y = L.T @ xp
    rhs = L @ y
    lower = np.abs(strict) @ np.abs(y) + np.abs(rhs) + np.abs(V) @ np.abs(Ld @ y)
    upper = np.abs(strict.T) @ np.abs(xp) + np.abs(y) + np.abs(V.T) @ np.abs(Ld.T @ xp)
    return float(max(lower.max(), upper.max())) * 2.0 ** (b - 1)
