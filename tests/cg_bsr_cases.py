"""Cases of cg_solve_bsr and the block-Jacobi routines (include/spmv/cg.h, include/spmv/bsr.h),
shared by tests/test_cg_bsr_host.py (no GPU) and tests/test_gpu_cg_bsr.py.

Exact systems by Kronecker lift.  A0 is exact_data.two_eig_system("cg", n0, L, scaled=False) with common diagonal
d = 2^14, K a unimodular SPD integer block and w a small integer vector: A = A0 (x) K, b = b0 (x) w.  The block diagonal
is d K, whose Cholesky factor is 128 L and whose inverse K^-1 / d is exact, so M^-1 A = (A0 / d) (x) I and block-Jacobi CG
ends after two steps with r = 0 (alpha = 2, 2 and beta = 1/2), at x1 = x1_0 (x) K^-1 w and x2 = x2_0 (x) K^-1 w.  With
K = I the same lift gives NONE's and JACOBI's bits.  The lift is built sparsely, straight into BSR arrays.

Float systems.  b unknowns per node on a scalar SPD pattern A0: A = Q^T (A0 (x) I_b) Q with Q = blockdiag(Q_I), every
Q_I = I + a strong random coupling, so block (I, J) is a_IJ Q_I^T Q_J: SPD by congruence, diagonal blocks far from
diagonal, and block-Jacobi sees D0^-1 A0 while scalar Jacobi sees the conditioning of the Q_I^T Q_I too.  Sizes that
are no multiple of b are leading principal submatrices.

Restatements in numpy of bsr_diag_inverse_cpu, bsr_diag_apply_cpu and of the iteration under cg.h's rules."""
import importlib

import numpy as np

import exact_data as ed

spd = importlib.import_module("gpu-spmv_amd.spd")

NONE, JACOBI, BLOCK_JACOBI = 0, 1, 2
BLOCK_DIMS = (2, 3, 4, 8)
LANES = ed.LANES
K_BLOCK = 256                                    # kBlock (csrc/device_common.h)
VEC_BLOCKS = 1024                                # kVecBlocks: the grid cap of cg_bsr_update and of the inverse kernel
ROW_BLOCKS = 2048                                # kMaxResidentBlocks: the grid cap of cg_bsr_spmv_dot / cg_bsr_init
SMALL_LIFTS = ((257, 1), (300, 4))               # (n0, L) of the smallest exact cases


def update_trip(b):
    """rows one trip of cg_bsr_update covers: its grid cap x T, T = kBlock - kBlock % b (255 for b = 3)"""
    return VEC_BLOCKS * (K_BLOCK - K_BLOCK % b)


def row_trip(lanes):
    """block rows one trip of the block-row kernels covers at a lane count"""
    return ROW_BLOCKS * K_BLOCK // lanes


# ------------------------------------------------------------------------------------------ the lift
def k_block(b, identity=False):
    """K[i][j] = min(i, j) + 1 = L L^T with L the unit lower all-ones triangle, for b = 8 too: there the largest row
    sum of |a||p| is 1.37e7 units of p's last bit against check_exact's 2^24 = 1.68e7 (tests/test_cg_bsr_host.py
    proves it for the smallest cases and prints the figure)."""
    if identity:
        return np.eye(b, dtype=np.int64)
    i = np.arange(b)
    return np.minimum(i[:, None], i[None, :]) + 1


def k_inverse(b, identity=False):
    """K^-1: the integer tridiagonal (2, -1; ...; last diagonal entry 1)"""
    if identity:
        return np.eye(b, dtype=np.int64)
    Ki = 2 * np.eye(b, dtype=np.int64) - np.eye(b, k=1, dtype=np.int64) - np.eye(b, k=-1, dtype=np.int64)
    Ki[-1, -1] = 1
    return Ki


def w_vector(b):
    return np.array([1, -2, 3, -1] * 2, np.int64)[:b]


_lift_cache = {}


def lifted_system(n0, L, b, identity):
    """dict(n, b, brp, bc, bv, rhs, x1, x2, rel1, inv): A = A0 (x) K as BSR arrays (block columns ascending), b = b0 (x) w,
    the iterates after one and two steps from x0 = 0, ||r1|| / ||b|| rounded to float32 from exact fp64 sums, and the
    inverses K^-1 / d of the diagonal blocks."""
    key = (n0, L, b, identity)
    if key in _lift_cache:
        return _lift_cache[key]
    s = ed.two_eig_system("cg", n0, L, scaled=False)
    rp0 = s["rp"].astype(np.int64)
    rows0 = np.repeat(np.arange(n0), np.diff(rp0))
    order = np.lexsort((s["ci"], rows0))                             # block columns ascending inside a block row
    ci0, va0 = s["ci"][order], s["va"][order]
    K, Ki, w = k_block(b, identity), k_inverse(b, identity), w_vector(b)
    assert np.array_equal(K @ Ki, np.eye(b, dtype=np.int64))
    bv = (va0[:, None] * K.ravel()[None, :].astype(np.float32)).astype(np.float32).ravel()
    kw = (Ki @ w).astype(np.float64)
    lift = lambda v0, v: (np.asarray(v0, np.float64)[:, None] * v[None, :]).ravel()
    rhs, x1, x2 = lift(s["b"], w.astype(np.float64)), lift(s["x1"], kw), lift(s["x2"], kw)
    # r1 = b - A x1 = (b0 - A0 x1_0) (x) w, every product and sum exact in fp64 (integers times dyadic fractions)
    r1_0 = s["b"].astype(np.float64) - spd.spmv64(rp0, ci0, va0, s["x1"])
    ww = float(np.dot(w, w))
    rel1 = np.float32(np.sqrt(np.sum(r1_0 * r1_0) * ww) / np.sqrt(np.sum(s["b"].astype(np.float64) ** 2) * ww))
    inv = np.tile((Ki.astype(np.float64) / ed.TWO_EIG_D).astype(np.float32).ravel(), n0)
    out = dict(n=n0 * b, n0=n0, b=b, L=L, brp=s["rp"].astype(np.int32), bc=ci0.astype(np.int32), bv=bv,
               rhs=(rhs + 0.0).astype(np.float32), x1=(x1 + 0.0).astype(np.float32), x2=(x2 + 0.0).astype(np.float32),
               rel1=rel1, inv=inv)
    while len(_lift_cache) >= 2:
        _lift_cache.pop(next(iter(_lift_cache)))
    _lift_cache[key] = out
    return out


def bsr_to_csr_arrays(n, b, brp, bc, bv):
    """(rp, ci, va) of every position of every block inside an n x n matrix (zeros kept), columns ascending"""
    brp = np.asarray(brp, np.int64)
    nb = bc.size
    block_row = np.repeat(np.arange(brp.size - 1), np.diff(brp))
    rows = (block_row[:, None, None] * b + np.arange(b)[None, :, None] + np.zeros((1, 1, b), np.int64)).ravel()
    cols = (np.asarray(bc, np.int64)[:, None, None] * b + np.zeros((1, b, 1), np.int64) + np.arange(b)[None, None, :]).ravel()
    vals = np.asarray(bv, np.float32).reshape(nb, b, b).ravel()
    keep = (rows < n) & (cols < n)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp, cols[order].astype(np.int32), vals[order]


# ------------------------------------------------------------------------------------------ float systems
def block_spd(n, b, seed, base="random", coupling=0.3):
    """(n, rp, ci, va): the leading n x n part of Q^T (A0 (x) I_b) Q (module docstring) as CSR, columns ascending"""
    n0 = -(-n // b)
    if base == "poisson3d":
        m = int(round(n0 ** (1.0 / 3.0)))
        while m ** 3 < n0:
            m += 1
        _, rp0, ci0, va0 = spd.poisson3d(m)
        keep0 = n0
    else:
        _, rp0, ci0, va0 = spd.random_spd(n0, 5, seed=seed)
        keep0 = n0
    rp0 = rp0.astype(np.int64)
    rows0 = np.repeat(np.arange(rp0.size - 1), np.diff(rp0))
    inside = (rows0 < keep0) & (ci0 < keep0)
    rows0, ci0, va0 = rows0[inside], ci0[inside].astype(np.int64), va0[inside].astype(np.float64)
    # repeated columns of random_spd add up: one entry per (row, column)
    key = rows0 * keep0 + ci0
    uniq, where = np.unique(key, return_inverse=True)
    va0 = np.bincount(where, weights=va0)
    rows0, ci0 = uniq // keep0, uniq % keep0
    rng = np.random.default_rng([seed, b, n])
    Q = np.eye(b)[None, :, :] + coupling * rng.uniform(-1.0, 1.0, size=(n0, b, b))
    blocks = va0[:, None, None] * np.einsum("eki,ekj->eij", Q[rows0], Q[ci0])       # a_IJ Q_I^T Q_J
    blocks = 0.5 * (blocks + np.einsum("eij->eji", blocks[np.searchsorted(uniq, ci0 * keep0 + rows0)]))
    rows = (rows0[:, None, None] * b + np.arange(b)[None, :, None] + np.zeros((1, 1, b), np.int64)).ravel()
    cols = (ci0[:, None, None] * b + np.zeros((1, b, 1), np.int64) + np.arange(b)[None, None, :]).ravel()
    vals = blocks.astype(np.float32).ravel()
    keep = (rows < n) & (cols < n)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    order = np.lexsort((cols, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return n, rp, cols[order].astype(np.int32), vals[order]


def ragged_sizes(b):
    """sizes of a few thousand rows that are no multiple of b (3k+1, 3k+2; 4k+3; 8k+5), and one that is"""
    return {2: (2001, 3000), 3: (2998, 2999, 3000), 4: (3003, 3000), 8: (3005, 3008)}[b]


def float_cases(b):
    """(n, base, seed) of the restatement-parity systems.  The seeds are chosen on the CPU alone: the relative residual
    a solve ends on is a quantity that two correct realisations of cg.h's iteration need not share to 1 %, the bound of
    test_gpu_cg.py, when the last steps hover at the tolerance, so every case here is one on which two realisations
    of the restatement agree to a quarter of that bound: the product rounded from fp64 sums against the product summed in
    fp32, against three copies with roundoff-sized noise on q and against the product in the lane-group kernel's
    documented order, restated on the CPU (reference_spread), and on which the restatement's last
    residual lies at least 5 % below the tolerance and the one before at least 5 % above it (stop_margin): a solve that
    stops one step earlier or later, as the +-2 steps of the bound allow, cannot end within 1 % of the reference's
    residual.  tests/test_cg_bsr_host.py asserts both."""
    seeds = FLOAT_SEEDS[b]
    return [(n, "poisson3d" if k == 1 else "random", seeds[k]) for k, n in enumerate(ragged_sizes(b))]


FLOAT_SEEDS = {2: (23, 25), 3: (23, 29, 23), 4: (38, 27), 8: (47, 68)}


def float_system(n, b, base, seed):
    n, rp, ci, va = block_spd(n, b, seed=seed, base=base)
    rhs = np.random.default_rng([n, seed]).uniform(-1.0, 1.0, n).astype(np.float32)
    return n, rp, ci, va, rhs


def spmv_fp32(rp, ci, va, x):
    """A x with fp32 products summed in fp32 (numpy's pairwise order): another correct realisation of q = A p"""
    rp = np.asarray(rp, np.int64)
    prod = (np.asarray(va, np.float32) * np.asarray(x, np.float32)[ci]).astype(np.float32)
    out = np.zeros(rp.size - 1, np.float32)
    nonempty = rp[1:] > rp[:-1]
    out[nonempty] = np.add.reduceat(prod, rp[:-1][nonempty])
    return out.astype(np.float64)


def spmv_noisy(seed):
    """q = A p rounded from fp64 sums, every entry then moved by up to one unit of fp32 roundoff of sum_j |a_ij| |p_j|,
    drawn from `seed`: the scale of the error of any fp32 summation order of the row (the measure conftest.reorder_err
    holds the reordering kernels to), which is what tells one correct realisation of the product from another"""
    rng = np.random.default_rng(seed)

    def product(rp, ci, va, x):
        q = spd.spmv64(rp, ci, va, x)
        scale = spd.spmv64(rp, ci, np.abs(va), np.abs(x))
        return q + rng.uniform(-1.0, 1.0, q.size) * 2.0 ** -24 * scale
    return product


def spmv_lane_order(n, b, rp, ci, va):
    """q = A p in the order cg_bsr_spmv_dot documents, on the CPU: the matrix as the blocks bsr_from_csr_cpu stores, the
    lane count of spmv_bsr's rule (the smallest L with 4 L >= 2 x the mean blocks per block row), lane l taking blocks
    l, l + L, ... of its block row with one fp32 multiply-add per entry, columns ascending inside a block, then the
    lanes' sums added pairwise (1 with 0, 3 with 2, ...; then the pairs).  Returns a product for restate(spmv=...)."""
    nb = -(-n // b)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    uniq, where = np.unique((rows // b) * nb + ci // b, return_inverse=True)
    bi, bj = uniq // nb, uniq % nb
    vals = np.zeros((uniq.size, b, b), np.float32)
    vals[where, rows % b, ci % b] = va
    brp = np.concatenate([[0], np.cumsum(np.bincount(bi, minlength=nb))])
    lanes = ed.lanes_for(2 * uniq.size, nb)
    pos = np.arange(uniq.size) - brp[bi]
    lane, step = pos % lanes, pos // lanes

    def product(rp_, ci_, va_, x):
        xp = np.zeros(nb * b, np.float32)
        xp[:n] = np.asarray(x, np.float32)
        xp = xp.reshape(nb, b)
        acc = np.zeros((nb, lanes, b), np.float32)
        for s in range(int(step.max()) + 1):
            sel = np.flatnonzero(step == s)
            a, xb = acc[bi[sel], lane[sel]], xp[bj[sel]]
            for c in range(b):
                fused = (vals[sel][:, :, c].astype(np.float64) * xb[:, c][:, None].astype(np.float64)
                         + a.astype(np.float64)).astype(np.float32)
                a = np.where((bj[sel] * b + c < n)[:, None], fused, a)
            acc[bi[sel], lane[sel]] = a
        while acc.shape[1] > 1:
            acc = (acc[:, 0::2, :] + acc[:, 1::2, :]).astype(np.float32)
        return acc[:, 0, :].ravel()[:n].astype(np.float64)
    return product


def reference_spread(n, b, rp, ci, va, rhs, tol, precond):
    """(largest relative difference of the final relative residual, largest difference of the iteration count) between
    the restatement and five other realisations of it: the product summed in fp32, three with roundoff-sized noise
    on q, and the product in the order the lane-group kernel documents (spmv_lane_order)"""
    first = restate(n, b, rp, ci, va, rhs, np.zeros(n), tol, 5000, precond)
    spread, steps = 0.0, 0
    for other in (spmv_fp32, spmv_noisy(1), spmv_noisy(2), spmv_noisy(3), spmv_lane_order(n, b, rp, ci, va)):
        second = restate(n, b, rp, ci, va, rhs, np.zeros(n), tol, 5000, precond, spmv=other)
        spread = max(spread, abs(first[4] - second[4]) / first[4])
        steps = max(steps, abs(first[1] - second[1]))
    return spread, steps


def stop_margin(n, b, rp, ci, va, rhs, tol, precond):
    """How far from the tolerance the restatement's stop is: min(1 - rel_k / tol, rel_{k-1} / tol - 1) for its last step
    k.  A realisation whose residuals stay within 1 % of the restatement's stops at the same step only if both sides
    are more than 1 % away; a solve that stops a step earlier or later cannot end on the same residual."""
    x, it, conv, brk, rel = restate(n, b, rp, ci, va, rhs, np.zeros(n), tol, 5000, precond)
    assert conv and it >= 2
    before = restate(n, b, rp, ci, va, rhs, np.zeros(n), 0.0, it - 1, precond)[4]
    tol = float(np.float32(tol))
    return min(1.0 - rel / tol, before / tol - 1.0)


STOP_MARGIN = 0.05                               # five times the 1 % the device is allowed


def dense_diagonal_blocks(n, b, rp, ci, va):
    """[num_block_rows, b, b] float32: the diagonal blocks of a CSR matrix, zeros where nothing is stored"""
    nb = -(-n // b)
    out = np.zeros((nb, b, b), np.float32)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    on = rows // b == ci // b
    out[rows[on] // b, rows[on] % b, ci[on] % b] = va[on]
    return out


# ------------------------------------------------------------------------------------------ restatements
def restate_inverse(n, b, blocks):
    """bsr.h's rule for every block of `blocks` [nb, b, b] float32 at once: (inv [nb * b * b] float32, ok [nb] bool).
    fp64, every operation rounded on its own; only the lower triangles are read."""
    nb = blocks.shape[0]
    size = np.minimum(b, n - np.arange(nb) * b)
    D = blocks.astype(np.float64)
    Lm = np.zeros((nb, b, b))
    ok = np.ones(nb, bool)
    with np.errstate(all="ignore"):
        for p in range(b):
            for q in range(p + 1):
                w = D[:, p, q].copy()
                for k in range(q):
                    w = w - Lm[:, p, k] * Lm[:, q, k]
                if q == p:
                    ok &= ~(p < size) | ((w > 0.0) & np.isfinite(w))
                    Lm[:, p, p] = np.sqrt(w)
                else:
                    Lm[:, p, q] = w / Lm[:, q, q]
        W = np.zeros((nb, b, b))
        for j in range(b):
            W[:, j, j] = 1.0 / Lm[:, j, j]
            for i in range(j + 1, b):
                t = np.zeros(nb)
                for k in range(j, i):
                    t = t + Lm[:, i, k] * W[:, k, j]
                W[:, i, j] = -t / Lm[:, i, i]
        inv = np.zeros((nb, b, b), np.float32)
        for i in range(b):
            for j in range(i + 1):
                s = np.zeros(nb)
                for k in range(i, b):
                    s = np.where(k < size, s + W[:, k, i] * W[:, k, j], s)
                v = np.where(i < size, s.astype(np.float32), np.float32(0.0)).astype(np.float32)
                inv[:, i, j] = v
                inv[:, j, i] = v
    return inv.ravel(), ok


def restate_apply(n, b, inv, r):
    """z = D^-1 r by the ordered sum, multiply and add rounded separately in float32"""
    nb = -(-n // b)
    inv = np.asarray(inv, np.float32).reshape(nb, b, b)
    rp = np.zeros(nb * b, np.float32)
    rp[:n] = r
    rp = rp.reshape(nb, b)
    z = np.zeros((nb, b), np.float32)
    with np.errstate(all="ignore"):
        for c in range(b):
            inside = (np.arange(nb) * b + c < n)[:, None]
            term = (inv[:, :, c] * rp[:, c][:, None]).astype(np.float32)
            z = np.where(inside, (z + term).astype(np.float32), z)
    return z.ravel()[:n]


def restate(n, b, rp, ci, va, rhs, x0, tol, max_iter=1000, precond=BLOCK_JACOBI, spmv=None):
    """numpy PCG under cg.h's numeric rules on the CSR expansion (test_gpu_cg.restate with a stored z); returns
    (x, iterations, converged, breakdown, relative residual)"""
    rhs = np.asarray(rhs, np.float32)
    x = np.asarray(x0, np.float32).copy()
    spmv32 = lambda v: (spmv or spd.spmv64)(rp, ci, va, v).astype(np.float32)
    if precond == BLOCK_JACOBI:
        inv, ok = restate_inverse(n, b, dense_diagonal_blocks(n, b, rp, ci, va))
        assert ok.all()
        apply = lambda r: restate_apply(n, b, inv, r)
    elif precond == JACOBI:
        blocks = dense_diagonal_blocks(n, b, rp, ci, va)
        d = blocks[:, np.arange(b), np.arange(b)].ravel()[:n]
        dinv = (np.float32(1.0) / d).astype(np.float32)
        apply = lambda r: (r * dinv).astype(np.float32)
    else:
        apply = lambda r: r.copy()
    dot = lambda a, c: float(np.dot(a.astype(np.float64), c.astype(np.float64)))
    r = (rhs - spmv32(x)).astype(np.float32)
    z = apply(r)
    p = z.copy()
    rz, rr, bb = dot(r, z), dot(r, r), dot(rhs, rhs)
    if bb == 0.0:
        return np.zeros(n, np.float32), 0, True, False, 0.0
    bnorm = np.sqrt(bb)
    thr = float(np.float32(tol)) * bnorm
    if np.sqrt(rr) <= thr:
        return x, 0, True, False, np.sqrt(rr) / bnorm
    if not rz > 0:
        return x, 0, False, True, np.sqrt(rr) / bnorm
    it, conv, brk, rel = 0, False, False, np.sqrt(rr) / bnorm
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


def true_residual(rp, ci, va, rhs, x):
    b64 = np.asarray(rhs, np.float64)
    return float(np.linalg.norm(b64 - spd.spmv64(rp, ci, va, x)) / np.linalg.norm(b64))


def helps_system():
    """(n, b, rp, ci, va, rhs): the float system of the 'BLOCK_JACOBI helps' tests: strongly coupled 4 x 4 blocks"""
    n, b = 3003, 4
    n, rp, ci, va = block_spd(n, b, seed=11, coupling=0.5)
    rhs = np.random.default_rng(5).uniform(-1.0, 1.0, n).astype(np.float32)
    return n, b, rp, ci, va, rhs


def forced(monkeypatch, lanes):
    monkeypatch.setenv("SPMV_DEBUG", "bsr_lanes=%d" % lanes)
