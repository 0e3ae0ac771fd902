"""The numpy restatement of include/spmv/gmres.h and the systems the GMRES tests share (tests/test_gmres_host.py on
the CPU, tests/test_gpu_gmres.py on the device).  A plain module, not a conftest.

restate() follows the header rule for rule: fp32 vectors, fp64 dot products of the fp32 entries, classical
Gram-Schmidt applied twice with the coefficients rounded to fp32 and applied by fmaf in ascending order, the
Hessenberg column h_i = double(fp32 h1_i) + double(fp32 h2_i), Givens rotations and the back-substitution in fp64,
u = sum fmaf(fp32 y_i, v_i, u), x += fp32(M^-1 u), and the residual recomputed at every close: the reported residual
IS the recomputed one.  Its dot products sum in numpy's order and its SpMV in the order `spmv` chooses; the device
has orders of its own, so trajectories are compared by measured bounds (test_gpu_gmres.py), never bit for bit."""
import importlib

import numpy as np

spd = importlib.import_module("gpu-spmv_amd.spd")
nonsym = importlib.import_module("gpu-spmv_amd.nonsym")

NONE, JACOBI = 0, 1
NO_BREAKDOWN, SINGULAR, NOT_FINITE = 0, 1, 2
RESTARTS = (1, 2, 7, 8, 9, 30, 64)          # every group-of-8 boundary of the basis walk, the default and the cap

# fp32 unit roundoff
U32 = 2.0 ** -24


def diag_of(n, rp, ci, va):
    """fp32 sum of the stored (i,i) entries in storage order (0 where a row has none)"""
    d = np.zeros(n, np.float32)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    for j in np.flatnonzero(ci == rows):
        d[rows[j]] = np.float32(d[rows[j]] + va[j])
    return d


def spmv_round_once(rp, ci, va, x):
    """row sums in fp64, rounded to fp32 once"""
    return spd.spmv64(rp, ci, va, x).astype(np.float32)


def spmv_sequential(rp, ci, va, x):
    """row sums in fp32, entry after entry in storage order, every product and sum rounded"""
    rp = np.asarray(rp, np.int64)
    n = rp.size - 1
    x = np.asarray(x, np.float32)
    acc = np.zeros(n, np.float32)
    lengths = np.diff(rp)
    for k in range(int(lengths.max()) if n else 0):
        rows = np.flatnonzero(lengths > k)
        at = rp[rows] + k
        acc[rows] = (acc[rows] + (va[at] * x[ci[at]]).astype(np.float32)).astype(np.float32)
    return acc


def fma(a, u, c):
    """fp32 fmaf(a, u, c) elementwise (the product of two fp32 values is exact in fp64)"""
    return (np.float64(a) * u.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def dot(a, c):
    return np.float64(np.dot(a.astype(np.float64), c.astype(np.float64)))


def true_residual(rp, ci, va, b, x):
    b64 = np.asarray(b, np.float64)
    return float(np.linalg.norm(b64 - spd.spmv64(rp, ci, va, x)) / np.linalg.norm(b64))


def residual_rounding_bound(rp, ci, va, b, x):
    """How far ||fp32(b - fp32-summed A x)|| / ||b|| can lie from the same figure in fp64: one SpMV's rounding.
    A row sum of L entries in ANY fp32 order, fused or not, errs by at most L u sum_j |a_ij x_j| (first order; L
    covers the L - 1 additions and the products), the subtraction by u |r_i|; the norms differ by at most the norm of
    the difference of the vectors."""
    rp = np.asarray(rp, np.int64)
    lengths = np.diff(rp)
    n = lengths.size
    rows = np.repeat(np.arange(n), lengths)
    absum = np.bincount(rows, weights=np.abs(va.astype(np.float64) * np.asarray(x, np.float64)[ci]), minlength=n)
    r = np.asarray(b, np.float64) - spd.spmv64(rp, ci, va, x)
    err = (lengths + 1) * U32 * absum + U32 * np.abs(r)
    return float(np.linalg.norm(err) / np.linalg.norm(np.asarray(b, np.float64)))


def restate(n, rp, ci, va, b, x0, tol=1e-6, max_iter=1000, restart=30, precond=JACOBI, spmv=spmv_round_once,
            apply_m=None):
    """GMRES(restart) under gmres.h's rules.  precond NONE / JACOBI, or apply_m(u) -> fp32 M^-1 u for a factorisation.
    Returns (x, iterations, restarts, converged, breakdown, relative residual)."""
    b = np.asarray(b, np.float32)
    x = np.asarray(x0, np.float32).copy()
    if apply_m is None and precond == JACOBI:
        dinv = (np.float32(1.0) / diag_of(n, rp, ci, va)).astype(np.float32)
        apply_m = lambda v: (v * dinv).astype(np.float32)
    elif apply_m is None:
        apply_m = lambda v: v
    iterations, cycles, breakdown = 0, 0, NO_BREAKDOWN
    final = False
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        bnorm = np.sqrt(bb)
        thr = np.float64(np.float32(tol)) * bnorm
        while True:
            # setup and every restart: the same code
            r = (b - spmv(rp, ci, va, x)).astype(np.float32)
            rr = dot(r, r)
            beta = np.sqrt(rr)
            if bb == 0:
                return np.zeros(n, np.float32), 0, 0, True, NO_BREAKDOWN, 0.0
            rel = float(np.float32(beta / bnorm))
            if not (np.isfinite(bb) and np.isfinite(rr)):
                return x, iterations, max(cycles - 1, 0), False, breakdown or NOT_FINITE, rel
            if beta <= thr:
                return x, iterations, max(cycles - 1, 0), True, breakdown, rel
            if final or iterations >= max_iter:
                return x, iterations, max(cycles - 1, 0), False, breakdown, rel
            cycles += 1
            V = [(r * np.float32(1.0 / beta)).astype(np.float32)]
            g = [np.float64(beta)]
            cs, sn, R = [], [], []
            k = 0
            for j in range(restart):
                w = spmv(rp, ci, va, apply_m(V[j]))
                h1 = [np.float32(dot(v, w)) for v in V]
                for hi, v in zip(h1, V):
                    w = fma(-hi, v, w)
                h2 = [np.float32(dot(v, w)) for v in V]
                for hi, v in zip(h2, V):
                    w = fma(-hi, v, w)
                col = [np.float64(a) + np.float64(c) for a, c in zip(h1, h2)]
                hn = np.sqrt(dot(w, w))
                for i in range(j):
                    a, c = col[i], col[i + 1]
                    col[i] = cs[i] * a + sn[i] * c
                    col[i + 1] = -sn[i] * a + cs[i] * c
                d = np.sqrt(col[j] * col[j] + hn * hn)
                if not (np.isfinite(hn) and np.isfinite(d) and all(np.isfinite(c) for c in col)):
                    breakdown, final = NOT_FINITE, True
                    break
                if d == 0:
                    breakdown, final = SINGULAR, True
                    break
                cs.append(col[j] / d)
                sn.append(hn / d)
                col[j] = d
                R.append(col)
                g.append(-sn[j] * g[j])
                g[j] = cs[j] * g[j]
                iterations += 1
                k = j + 1
                if iterations >= max_iter:
                    final = True
                if abs(g[j + 1]) <= thr or k == restart or iterations >= max_iter or hn == 0:
                    break
                V.append((w * np.float32(1.0 / hn)).astype(np.float32))
            # close: R y = g, u, x
            if k > 0:
                y = [np.float64(0)] * k
                for i in range(k - 1, -1, -1):
                    s = g[i]
                    for l in range(i + 1, k):
                        s = s + -(R[l][i] * y[l])
                    y[i] = s / R[i][i]
                u = np.zeros(n, np.float32)
                for i in range(k):
                    u = fma(np.float32(y[i]), V[i], u)
                x = (x + apply_m(u)).astype(np.float32)


def krylov_optimum(n, rp, ci, va, b, k, precond=JACOBI):
    """min over the k-dimensional Krylov space of A M^-1 and b (x0 = 0) of ||b - A M^-1 t|| / ||b||, in fp64"""
    b = np.asarray(b, np.float64)
    dinv = 1.0 / diag_of(n, rp, ci, va).astype(np.float64) if precond == JACOBI else np.ones(n)
    op = lambda v: spd.spmv64(rp, ci, va, v * dinv)
    Q = np.zeros((n, 0))
    v = b / np.linalg.norm(b)
    for _ in range(k):                               # an orthonormal basis of the space, by repeated projection
        for _ in range(2):
            v = v - Q @ (Q.T @ v)
        if np.linalg.norm(v) < 1e-13:
            break
        v = v / np.linalg.norm(v)
        Q = np.column_stack([Q, v])
        v = op(v)
    AQ = np.column_stack([op(Q[:, i]) for i in range(Q.shape[1])])
    t, *_ = np.linalg.lstsq(AQ, b, rcond=None)
    return float(np.linalg.norm(b - AQ @ t) / np.linalg.norm(b))


def random_system(n, seed=0):
    """random_nonsym with a quarter of the rows negated (k = min(7, n - 1) off-diagonal entries per row)"""
    if n == 1:
        return 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-2.5], np.float32)
    return nonsym.random_nonsym(n, min(7, n - 1), seed=seed + n, negative_rows=0.25)


SYSTEMS = {
    "random_1": lambda: random_system(1),
    "random_2": lambda: random_system(2),
    "random_63": lambda: random_system(63),
    "random_64": lambda: random_system(64),
    "random_65": lambda: random_system(65),
    "random_257": lambda: random_system(257),
    "convdiff2d_16": lambda: nonsym.convdiff2d(16, 2.0),
    "convdiff2d_64": lambda: nonsym.convdiff2d(64, 5.0),
}


def rhs(n, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
