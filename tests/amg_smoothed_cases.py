"""Shared helpers of tests/test_amg_smoothed_host.py, tests/test_gpu_amg_smoothed.py and
tests/test_gpu_cg_amg_smoothed.py: numpy restatements of the smoothed-aggregation part of include/spmv/amg.h (the
hierarchy through the host twins spgemm_cpu_csr, csr_scale_cpu and csr_add_cpu with theta decaying per level, the
weighted V-cycle in fp32 and in fp64) and an exact prover of the two transfers.  A plain module, not a conftest."""
from fractions import Fraction

import numpy as np

import amg_cases as ac
from amg_cases import NotExact, Prover


# ---- matrices ------------------------------------------------------------------------------------------------
def arrow(n=300):
    """a_00 = 1024, a_0j = a_j0 = -1, a_jj = 4: with omega_p = 1/2 every s_i is a power of two, and row 0 of P and of
    P^T (singleton aggregates) has n entries"""
    rows, cols, vals = [0] * n, list(range(n)), [1024.0] + [-1.0] * (n - 1)
    for j in range(1, n):
        rows += [j, j]
        cols += [0, j]
        vals += [-1.0, 4.0]
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, np.asarray(cols, np.int32), np.asarray(vals, np.float32)


def block_map(n, size):
    """aggregates of `size` consecutive rows"""
    assert n % size == 0
    return (np.arange(n) // size).astype(np.int32)


# ---- one level -------------------------------------------------------------------------------------------------
def scale_of(n, rp, ci, va, weight):
    """s_i = float(-double(omega_p) / double(d_i))"""
    d = ac.diag32(n, rp, ci, va).astype(np.float64)
    return (-np.float64(np.float32(weight)) / d).astype(np.float32)


def prolongator(spmv, n, rp, ci, va, agg, count, weight):
    """P = csr_add(1, T, 1, csr_scale(spgemm(A, T), rows = s)) through the host twins: (row_ptrs, cols, vals)"""
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    T = spmv.csr_from_arrays(n, count, *ac.prolongation(n, agg))
    AT, P, S = spmv.csr_create(0, 0, 0), spmv.csr_create(0, 0, 0), None
    try:
        assert spmv.spgemm_cpu_csr(AT, A, T) == 0
        status, scaled = spmv.csr_scale_cpu(AT, scale_of(n, rp, ci, va, weight), None)
        assert status == 0
        at_rp, at_ci, _ = spmv.csr_host_arrays(AT)
        S = spmv.csr_from_arrays(n, count, at_rp, at_ci, scaled)
        assert spmv.csr_add_cpu(P, 1.0, T, 1.0, S) == 0
        return spmv.csr_host_arrays(P)
    finally:
        for M in (A, T, AT, P, S):
            spmv.csr_destroy(M)


def transpose(rows, cols, rp, ci, va):
    """the CSR transpose in csr_transpose_gpu's stable order: inside a row of the result the source rows ascend"""
    ci = np.asarray(ci, np.int64)
    order = np.argsort(ci, kind="stable")
    out_rp = np.zeros(cols + 1, np.int32)
    np.cumsum(np.bincount(ci, minlength=cols), out=out_rp[1:])
    return out_rp, ac.rows_of(rows, rp)[order].astype(np.int32), np.asarray(va, np.float32)[order]


def galerkin(spmv, n, rp, ci, va, count, P, PT):
    """spgemm(PT, spgemm(A, P)) on the host"""
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    Pm = spmv.csr_from_arrays(n, count, *P)
    PTm = spmv.csr_from_arrays(count, n, *PT)
    AP, C = spmv.csr_create(0, 0, 0), spmv.csr_create(0, 0, 0)
    try:
        assert spmv.spgemm_cpu_csr(AP, A, Pm) == 0 and spmv.spgemm_cpu_csr(C, PTm, AP) == 0
        assert (C.contents.num_rows, C.contents.num_cols) == (count, count)
        return spmv.csr_host_arrays(C)
    finally:
        for M in (A, Pm, PTm, AP, C):
            spmv.csr_destroy(M)


# ---- hierarchy -----------------------------------------------------------------------------------------------
def mis2_aggregate(spmv, seed=0):
    """the aggregation amg_setup_smoothed_device uses, from its host definition"""
    def run(n, rp, ci, va, theta):
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        status, agg, count, _ = spmv.amg_aggregate_mis2_cpu_csr(A, theta, seed)
        spmv.csr_destroy(A)
        assert status == 0 and (agg >= 0).all()
        return agg, count
    return run


def hierarchy(spmv, n, rp, ci, va, theta=0.08, coarse_rows=64, max_levels=10, maps=None, weight=2.0 / 3.0, decay=0.5,
              aggregate=None):
    """The levels amg_setup_smoothed builds, restated: amg_cases.hierarchy's dicts plus P and PT (row_ptrs, cols, vals)
    and theta, the threshold the level's aggregation took."""
    aggregate = aggregate or ac.aggregate
    theta = np.float32(theta)
    levels = []
    while True:
        level = dict(n=n, rp=np.asarray(rp, np.int32), ci=np.asarray(ci, np.int32), va=np.asarray(va, np.float32),
                     agg=None, count=0, P=None, PT=None, theta=theta)
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
        level["P"] = prolongator(spmv, n, rp, ci, va, agg, count, weight)
        level["PT"] = transpose(n, count, *level["P"])
        rp, ci, va = galerkin(spmv, n, rp, ci, va, count, level["P"], level["PT"])
        n = count
        theta = np.float32(theta * np.float32(decay))


# ---- the weighted V-cycle in numpy -----------------------------------------------------------------------------
def _matvec(rows, csr, x, dtype):
    return ac._spmv(dict(n=rows, rp=csr[0], ci=csr[1], va=csr[2]), x, dtype)


def vcycle(levels, r, omega=2.0 / 3.0, pre=1, post=1, coarse_sweeps=4, dtype=np.float64, l=0):
    """One V-cycle on a smoothed hierarchy from a zero guess, every operation in `dtype`; the smoother and the
    coarsest level are amg_cases.vcycle's."""
    level = levels[l]
    if l == len(levels) - 1:
        return ac.vcycle([level], r, omega, pre, post, coarse_sweeps, dtype)
    n = level["n"]
    f = np.asarray(r, dtype)
    wd = np.float64(np.float32(omega)) / ac.diag32(n, level["rp"], level["ci"], level["va"]).astype(np.float64)
    wd = wd.astype(np.float32).astype(dtype) if dtype == np.float32 else wd
    sweep = lambda x: (x + wd * (f - ac._spmv(level, x, dtype))).astype(dtype)
    x = (wd * f).astype(dtype)
    for _ in range(pre - 1):
        x = sweep(x)
    res = (f - ac._spmv(level, x, dtype)).astype(dtype)
    fc = _matvec(level["count"], level["PT"], res, dtype)
    e = vcycle(levels, fc, omega, pre, post, coarse_sweeps, dtype, l + 1)
    x = (x + _matvec(n, level["P"], e, dtype)).astype(dtype)
    for _ in range(post):
        x = sweep(x)
    return x


# ---- the exact prover of the transfers -------------------------------------------------------------------------
def _rows(count, csr):
    rp, ci, va = csr
    return [[(int(ci[p]), Fraction(float(va[p]))) for p in range(rp[i], rp[i + 1])] for i in range(count)]


def prove_transfers(level, f, x, e):
    """(f_coarse, x_out, bits) as float32 arrays when every sum of amg_restrict(f, x) and amg_prolong(e, x) on this
    level is exact in fp32 whatever order the lanes take (Prover's rule: every term a multiple of one power-of-two
    quantum q and sum |terms| < 2^24 q), else (None, None, reason).  The residual's terms are f_i and the products
    of row i of A; the restriction's are those of row a of PT with the residuals; the prolongation's are x_i and the
    products of row i of P."""
    n, count = level["n"], level["count"]
    prover = Prover()
    f, x, e = ([Fraction(int(v)) for v in vec] for vec in (f, x, e))
    try:
        A = _rows(n, (level["rp"], level["ci"], level["va"]))
        res = [prover.total([f[i]] + [-a * x[j] for j, a in A[i]]) for i in range(n)]
        fc = [prover.total([w * res[i] for i, w in row]) for row in _rows(count, level["PT"])]
        out = [prover.total([x[i]] + [w * e[a] for a, w in row]) for i, row in enumerate(_rows(n, level["P"]))]
    except NotExact as why:
        return None, None, str(why)
    as32 = lambda vec: np.array([float(v) for v in vec], np.float32)
    assert all(Fraction(float(a)) == b for a, b in zip(as32(fc), fc))
    assert all(Fraction(float(a)) == b for a, b in zip(as32(out), out))
    return as32(fc), as32(out), prover.bits


def exact_vectors(level, seed=5):
    """integer f, x (n) and e (count) in [-8, 8]"""
    rng = np.random.default_rng(seed)
    draw = lambda m: rng.integers(-8, 9, m).astype(np.float32)
    return draw(level["n"]), draw(level["n"]), draw(level["count"])
