"""The numpy restatement of include/spmv/eigs.h and the matrices the eigs tests share (tests/test_eigs_host.py on the
CPU, tests/test_gpu_eigs.py on the device).  A plain module, not a conftest.

jacobi() is sym_eig_small's rule operation for operation: every numpy fp64 product, sum, quotient and root is rounded
separately, as the host twin and the device kernel round theirs, so all three give the same bits.  restate() follows
eigs_sym rule for rule: fp32 vectors, fp64 dot products of the fp32 entries, classical Gram-Schmidt applied twice with
the coefficients rounded to fp32 and applied by fmaf in ascending order, the dense projected matrix T, the Ritz
decomposition by jacobi(), the estimates, the thick restart and the finish with RECOMPUTED residuals.  Its dot products
sum in numpy's order and its SpMV in the order `spmv` chooses; the device has orders of its own, so runs on general
data are compared by measured bounds.  Where the data make every order give the same bits (one-hot systems up to the
first close, the first step of an integer system) tests/test_gpu_eigs_exact.py holds the device to restate() bit for bit.

Measured on the CPU (restate() against fp64 eigh, tolerance 1e-5, max_iterations 6000, the CASES and SHAPES below, both
ends of the spectrum: 50 runs; `python tests/eigs_cases.py` prints the table and `--write-golden` records the runs in
tests/golden/eigs_restate.json, which the GPU tier compares against).  Worst figures over all runs, relative to
max |lambda| where that applies:
    every run converges: converged == k, in 32 .. 1914 steps (the long ones are (k, m) = (7, 9) at the SMALLEST end:
                         a thick restart there keeps 8 of 9 vectors, one new column per cycle)
    value error / max|lambda|                      1.5e-7
    max |Y^T Y - I|                                3.8e-7 ((7, 9): 8.7e-6 after up to 1905 restarts)
    |fp32 residual - fp64 residual| / max|lambda|  4.0e-8 (the honesty of the recomputed residual)
and between two SpMV summation orders (spmv_round_once against spmv_sequential), the way GMRES's spread was measured:
    value difference / max|lambda|                 1.3e-7
    max_residual difference / max|lambda|          1.2e-6 on the simple spectra
    iteration count difference                     0, once 1 (of 1080) on the simple spectra; up to 24 steps (two
                                                   cycles at (8, 32)) on poisson3d(8), whose spectrum is degenerate:
                                                   which copy of a multiple eigenvalue a run finds first is decided by
                                                   rounding
The GPU tier is held to 4 x these figures (the constants below).  An iteration count is compared in units it can
move by: the estimates are tested at cycle closes only, so the unit is one cycle's new columns, m - p.
The floor: at tolerance 1e-6 every run converges except (7, 9) SMALLEST on the two indefinite matrices (4 and 2 of 7
pairs after 6000 steps); at 3e-7 seven runs fail, all of them (7, 9); every other shape still converges at 3e-7.  So
1e-5, the default, is the smallest tested tolerance at which all listed cases converge, and a basis with m >= 2k keeps
converging down to 3e-7.  See DESIGN.md section 4.20.

Measured for jacobi() itself against numpy.linalg.eigh over ORDERS x small_matrices(), relative to max |T_ij| (1 for the
zero matrix): see SMALL_* below and test_eigs_host.py, which prints the figures it measures.
"""
import importlib

import numpy as np

import gmres_cases as gc

spd = importlib.import_module("gpu-spmv_amd.spd")
synth = importlib.import_module("gpu-spmv_amd.synth")

LARGEST, SMALLEST = 0, 1
NO_BREAKDOWN, INVARIANT_SUBSPACE, NOT_FINITE = 0, 1, 2
START_SEED, START_TAG = 0x45494753, 0
MAX_ORDER, MAX_SWEEPS = 64, 30

ORDERS = (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64)
SHAPES = ((1, 8), (4, 20), (8, 32), (7, 9), (32, 64))          # (k, m)

# 4 x the figures of the module docstring
VALUE_BOUND = 4 * 1.5e-7
ORTHO_BOUND = 4 * 3.8e-7
ORTHO_BOUND_7_9 = 4 * 8.7e-6
HONESTY_MEASURED = 4.0e-8                  # recorded only: the tests use residual_rounding_bound, a model
RESIDUAL_SPREAD = 4 * 1.2e-6              # max_residual between two summation orders, simple spectra
DEGENERATE_ITERATION_SPREAD = 4 * 24
TOLERANCE = 1e-5
MAX_ITERATIONS = 6000
# jacobi() against eigh: measured 9.4e-14 / 3.2e-14 / 1.8e-14 (values, T S - S Theta, S^T S - I; worst over ORDERS x
# small_matrices(), relative to max |T_ij|; at most 14 sweeps), x 4
SMALL_VALUE_BOUND = 4 * 9.4e-14
SMALL_RESIDUAL_BOUND = 4 * 3.2e-14
SMALL_ORTHO_BOUND = 4 * 1.8e-14
GOLDEN = "eigs_restate.json"


def ortho_bound(k, m):
    return ORTHO_BOUND_7_9 if (k, m) == (7, 9) else ORTHO_BOUND


def iteration_bound(name, k, m):
    """How far an iteration count may lie from the recorded restatement's: 4 x the measured spread, which on the
    simple spectra is one unit (measured 0 and 1 step; the unit is what a straddled threshold costs)."""
    return 4 * iteration_spread(k, m) if name in SIMPLE_SPECTRA else max(DEGENERATE_ITERATION_SPREAD,
                                                                          4 * iteration_spread(k, m))


def iteration_spread(k, m):
    """one cycle's new columns: the estimates are tested at cycle closes only, so two runs whose estimates straddle the
    threshold at one close differ by the m - p steps of one more cycle"""
    return m - min(k + (m - k) // 2, m - 1)


# ---- sym_eig_small ----------------------------------------------------------------------------------------------------

def round_robin_pairs(r, N):
    pairs = [(r, N - 1)] + [((r + i) % (N - 1), (r - i + N - 1) % (N - 1)) for i in range(1, N // 2)]
    return [(min(a, b), max(a, b)) for a, b in pairs]


def jacobi(T):
    """(values ascending, vectors with eigenvector i in ROW i, sweeps) by eigs.h's rule"""
    W = np.array(T, np.float64)
    n = W.shape[0]
    S = np.eye(n)
    scale = np.max(np.abs(W)) if n else 0.0
    thr = scale * 2.0 ** -53
    N = (n + 1) & ~1
    sweeps = 0
    with np.errstate(all="ignore"):
        for sweep in range(MAX_SWEEPS):
            rotated = False
            sweeps += 1
            for r in range(N - 1):
                pairs = [(p, q) for p, q in round_robin_pairs(r, N) if q < n and abs(W[p, q]) > thr]
                if not pairs:
                    continue
                rotated = True
                p = np.array([a for a, _ in pairs])
                q = np.array([b for _, b in pairs])
                apq = W[p, q]
                tau = (W[q, q] - W[p, p]) / (2.0 * apq)
                root = np.sqrt(1.0 + tau * tau)
                t = np.where(tau < 0.0, -1.0, 1.0) / (np.abs(tau) + root)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                for M in (W, S):                                    # columns
                    x, y = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * x - s * y
                    M[:, q] = s * x + c * y
                x, y = W[p, :].copy(), W[q, :].copy()               # rows
                W[p, :] = c[:, None] * x - s[:, None] * y
                W[q, :] = s[:, None] * x + c[:, None] * y
                W[p, q] = 0.0
                W[q, p] = 0.0
            if not rotated:
                break
    d = np.diag(W).copy()
    order = np.argsort(d, kind="stable")
    return d[order], S[:, order].T.copy(), sweeps


def small_matrices(n, seed=0):
    """name -> symmetric fp64 matrix of order n"""
    rng = np.random.default_rng(1000 * n + seed)
    R = rng.uniform(-1.0, 1.0, (n, n))
    out = {"random": (R + R.T) / 2.0, "diagonal": np.diag(rng.uniform(-3.0, 3.0, n)), "zero": np.zeros((n, n))}
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = rng.uniform(-1.0, 1.0, n)
    lam[: (n + 1) // 2] = 0.75                                       # a repeated eigenvalue
    rep = (Q * lam) @ Q.T
    out["repeated"] = (rep + rep.T) / 2.0
    arrow = np.diag(np.sort(rng.uniform(1.0, 2.0, n))[::-1].copy())   # what a thick restart leaves: diag + a last
    if n > 1:                                                         # row / column that has already converged
        arrow[n - 1, : n - 1] = arrow[: n - 1, n - 1] = rng.uniform(-1.0, 1.0, n - 1) * 1e-9
    out["arrowhead"] = arrow
    return out


# ---- eigs_sym ---------------------------------------------------------------------------------------------------------

def default_start(n):
    return synth.vector(START_SEED, START_TAG, n)


def default_basis(k, n):
    return min(min(max(2 * k, 20), MAX_ORDER), n)


def sort_ritz(values, vectors, which):
    """eigs.h's order: descending for LARGEST, ascending for SMALLEST, equal values by ascending position"""
    keys = -values if which == LARGEST else values
    order = np.argsort(keys, kind="stable")
    return values[order], vectors[order]


def rotate(C, V):
    """row i = fp32(sum over l ascending of double(C[i, l]) * double(V[l])), every partial sum in fp64"""
    acc = np.zeros((C.shape[0], V.shape[1]), np.float64)
    C64, V64 = C.astype(np.float64), V.astype(np.float64)
    for l in range(V.shape[0]):
        acc = acc + C64[:, l:l + 1] * V64[l]
    return acc.astype(np.float32)


def residual32(rp, ci, va, theta, y, spmv):
    """eigs.h's recomputed residual: the fp64 norm of d_e = fmaf(-fp32(theta), y_e, (A y)_e)"""
    d = gc.fma(-np.float32(theta), y, spmv(rp, ci, va, y))
    return float(np.sqrt(gc.dot(d, d)))


def restate(n, rp, ci, va, k, which=LARGEST, m=0, tol=1e-5, max_iter=1000, v0=None, spmv=gc.spmv_round_once):
    """eigs_sym under eigs.h's rules.  Returns a dict: values, vectors (k x n), residuals (fp32; NaN / zero rows for
    the pairs not returned), found, converged, iterations, restarts, breakdown, max_residual."""
    m = min(m if m else min(max(2 * k, 20), MAX_ORDER), n)
    tol64 = np.float64(np.float32(tol))
    out = {"values": np.full(k, np.nan, np.float32), "residuals": np.full(k, np.nan, np.float32),
           "vectors": np.zeros((k, n), np.float32), "found": 0, "converged": 0, "iterations": 0, "restarts": 0,
           "breakdown": NO_BREAKDOWN, "max_residual": 0.0}
    start = np.asarray(default_start(n) if v0 is None else v0, np.float32)
    with np.errstate(all="ignore"):
        beta0 = np.sqrt(gc.dot(start, start))
        if not np.isfinite(beta0):
            out.update(breakdown=NOT_FINITE, max_residual=float("nan"))
            return out
        if beta0 == 0:
            raise ValueError("zero start vector: INVALID_ARGUMENT")
        V = np.zeros((m + 1, n), np.float32)
        V[0] = (start * np.float32(1.0 / beta0)).astype(np.float32)
        T = np.zeros((m, m), np.float64)
        c, iterations, restarts = 0, 0, 0
        beta = np.float64(0.0)
        while True:
            invariant = False
            while c < m and iterations < max_iter and not invariant:           # the steps of one cycle
                j = c
                w = spmv(rp, ci, va, V[j])
                h1 = [np.float32(gc.dot(V[i], w)) for i in range(j + 1)]
                for i in range(j + 1):
                    w = gc.fma(-h1[i], V[i], w)
                h2 = [np.float32(gc.dot(V[i], w)) for i in range(j + 1)]
                for i in range(j + 1):
                    w = gc.fma(-h2[i], V[i], w)
                h = np.array([np.float64(a) + np.float64(b) for a, b in zip(h1, h2)])
                beta = np.sqrt(gc.dot(w, w))
                if not (np.isfinite(beta) and np.all(np.isfinite(h))):
                    out.update(breakdown=NOT_FINITE, iterations=iterations, restarts=restarts,
                               max_residual=float("nan"))
                    return out
                T[: j + 1, j] = h
                T[j, : j + 1] = h
                iterations += 1
                c = j + 1
                invariant = bool(beta <= np.max(np.abs(h)) * 2.0 ** -20) or c == n
                if not invariant:
                    V[c] = (w * np.float32(1.0 / beta)).astype(np.float32)
            # the close
            cap = iterations >= max_iter
            found = min(k, c)
            if c > 0:
                values, vectors, _ = jacobi(T[:c, :c])
                theta, S = sort_ritz(values, vectors, which)                   # S[i] = Ritz vector i in the basis
                theta_max = np.max(np.abs(theta))
                estimates = np.abs(beta * S[:, c - 1])
                passing = c >= k and bool(np.all(estimates[:k] <= tol64 * theta_max))
                C = S.astype(np.float32)
            else:
                theta, theta_max, passing = np.zeros(0), 0.0, False
            p = min(k + (m - k) // 2, c - 1)
            if passing or cap or invariant:                                     # finish
                Y = rotate(C[:found, :c], V[:c]) if found else np.zeros((0, n), np.float32)
                res = np.array([residual32(rp, ci, va, theta[i], Y[i], spmv) for i in range(found)])
                converged = int(np.sum(res <= tol64 * theta_max))
                out["values"][:] = np.nan
                out["residuals"][:] = np.nan
                out["vectors"][:] = 0
                out["values"][:found] = theta[:found].astype(np.float32)
                out["residuals"][:found] = res.astype(np.float32)
                out["vectors"][:found] = Y
                out.update(found=found, converged=converged, iterations=iterations, restarts=restarts,
                           max_residual=float(res.max()) if found else 0.0)
                if converged == k or cap or invariant:
                    if invariant and found < k:
                        out["breakdown"] = INVARIANT_SUBSPACE
                    return out
            # thick restart
            Vnew = rotate(C[:p, :c], V[:c])
            nxt = V[c].copy()
            V[:p] = Vnew
            V[p] = nxt
            T[:] = 0.0
            T[np.arange(p), np.arange(p)] = theta[:p]
            c = p
            restarts += 1


# ---- the matrices -----------------------------------------------------------------------------------------------------

def shifted(system, shift):
    n, rp, ci, va = system
    va = va.copy()
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    va[ci == rows] = (va[ci == rows] - np.float32(shift)).astype(np.float32)
    return n, rp, ci, va


CASES = {
    "random_500": lambda: spd.random_spd(500, 7, seed=3),
    "random_1025": lambda: spd.random_spd(1025, 7, seed=5),
    "indefinite_500": lambda: shifted(spd.random_spd(500, 7, seed=3), 8.0),
    "indefinite_1025": lambda: shifted(spd.random_spd(1025, 7, seed=5), 8.0),
    "poisson3d_8": lambda: spd.poisson3d(8),
}
SIMPLE_SPECTRA = ("random_500", "random_1025", "indefinite_500", "indefinite_1025")   # the k extreme values are demanded
MIN_RELATIVE_GAP = 1e-4

_dense_cache = {}


def dense(name):
    """(system, fp64 dense matrix, ascending eigenvalues, eigenvectors in columns), computed once per case"""
    if name not in _dense_cache:
        system = CASES[name]()
        n, rp, ci, va = system
        D = np.zeros((n, n), np.float64)
        rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
        np.add.at(D, (rows, ci), va.astype(np.float64))
        lam, Q = np.linalg.eigh(D)
        _dense_cache[name] = (system, D, lam, Q)
    return _dense_cache[name]


def wanted(lam, k, which):
    """the k extreme eigenvalues in eigs.h's order"""
    return lam[::-1][:k] if which == LARGEST else lam[:k]


def extreme_gap(lam, k, which):
    """the smallest distance between neighbours among the k + 1 extreme eigenvalues, relative to the spectrum's width"""
    ext = wanted(lam, min(k + 1, lam.size), which)
    return float(np.min(np.abs(np.diff(ext))) / (lam[-1] - lam[0])) if ext.size > 1 else np.inf


def fp64_residuals(D, values, vectors):
    """||A y - theta y||_2 in fp64 for the returned fp32 pairs"""
    Y = vectors.astype(np.float64)
    return np.linalg.norm(D @ Y.T - Y.T * values.astype(np.float64), axis=0)


def residual_rounding_bound(rp, ci, va, theta, y):
    """How far the device's fp32 residual norm can lie from the fp64 one: one SpMV's rounding (a row sum of L entries in
    any fp32 order errs by at most L u sum |a_ij y_j|) and the one rounding of the fmaf (u |d_i|); gmres_cases.
    residual_rounding_bound is the model."""
    rp = np.asarray(rp, np.int64)
    lengths = np.diff(rp)
    n = lengths.size
    rows = np.repeat(np.arange(n), lengths)
    y64 = np.asarray(y, np.float64)
    absum = np.bincount(rows, weights=np.abs(va.astype(np.float64) * y64[ci]), minlength=n)
    d = spd.spmv64(rp, ci, va, y) - float(theta) * y64
    return float(np.linalg.norm(lengths * gc.U32 * absum + gc.U32 * np.abs(d)))


def run_case(job):
    """one line of the table: restate() against fp64 for (name, k, m, which, sequential)"""
    name, k, m, which, sequential = job
    (n, rp, ci, va), D, lam, Q = dense(name)
    lmax = float(np.max(np.abs(lam)))
    a = restate(n, rp, ci, va, k, which, m, tol=TOLERANCE, max_iter=MAX_ITERATIONS,
                spmv=gc.spmv_sequential if sequential else gc.spmv_round_once)
    near = np.array([np.min(np.abs(lam - v)) for v in a["values"].astype(np.float64)])
    err = np.abs(a["values"] - wanted(lam, k, which)) if name in SIMPLE_SPECTRA else near
    Y = a["vectors"].astype(np.float64)
    honest = np.abs(fp64_residuals(D, a["values"], a["vectors"]) - a["residuals"])
    return {"key": "%s|%d|%d|%d" % (name, k, m, which), "sequential": sequential, "iterations": a["iterations"],
            "restarts": a["restarts"], "converged": a["converged"], "max_residual": a["max_residual"] / lmax,
            "value_error": float(err.max() / lmax), "ortho": float(np.max(np.abs(Y @ Y.T - np.eye(k)))),
            "honesty": float(honest.max() / lmax), "values": [float(v) for v in a["values"]]}


def golden_key(name, k, m, which):
    return "%s|%d|%d|%d" % (name, k, m, which)


if __name__ == "__main__":          # the table of the module docstring; --write-golden records the round-once runs
    import json
    import multiprocessing
    import os
    import sys

    jobs = [(name, k, m, which, seq) for name in CASES for k, m in SHAPES for which in (LARGEST, SMALLEST)
            for seq in (0, 1)]
    with multiprocessing.Pool(min(12, os.cpu_count() or 1)) as pool:
        rows = pool.map(run_case, jobs)
    first = {r["key"]: r for r in rows if not r["sequential"]}
    second = {r["key"]: r for r in rows if r["sequential"]}
    for key in first:
        a, b = first[key], second[key]
        print(key, a["iterations"], b["iterations"], a["restarts"], a["converged"], b["converged"],
              "%.2e %.2e %.2e %.2e" % (a["value_error"], a["ortho"], a["max_residual"], a["honesty"]),
              "spread %.2e %.2e" % (max(abs(x - y) for x, y in zip(a["values"], b["values"])),
                                    abs(a["max_residual"] - b["max_residual"])))
    for field in ("value_error", "ortho", "honesty"):
        print(field, max(max(r[field] for r in first.values()), max(r[field] for r in second.values())))
    if "--write-golden" in sys.argv:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
        with open(path, "w") as f:
            json.dump({key: {"iterations": r["iterations"], "restarts": r["restarts"],
                             "max_residual": r["max_residual"]} for key, r in sorted(first.items())}, f, indent=1)
            f.write("\n")
