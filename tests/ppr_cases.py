"""Personalized PageRank (include/spmv/pagerank.h pagerank_personalized) without a GPU: the integer prover of

    s        = float(sum of r_old over the dangling nodes)
    r_new[i] = (d * (A r_old)[i] + (d * s) * v[i]) + (1 - d) * v[i],        r_0 = v

for a teleport vector v that is uniform over a power-of-two number of seed nodes, the catalogue of graphs and seed
sets the GPU tests run, and a float64 power iteration for graphs that are not exact.

The prover generalises exact_data._dyadic_run (v = 1 / n there): n a power of two, a dyadic damping factor, every
stored value 2^-j.  Every quantity of a step is then a dyadic rational, and while each of them fits float32's 24 bits
every summation order and every rounding gives the same bits.  It checks, per step: every product and row sum (one
quantum per row, the sum below 2^24 of them); s, d * acc, d * s, (d * s) * v, (1 - d) * v, both partial sums, r_new and
r_new - r_old representable in float32; the mass exactly 1.  It also models the residual the device reports: each
(r_new - r_old)^2 rounded to float32, their sum in fp64 (exact in any order when the squares share a quantum and the
sum stays below 2^53 of it: that is checked too), one correctly rounded square root, one rounding to float32.

A plain module, imported by tests/test_ppr_prover.py and tests/test_gpu_ppr.py; exact_data is imported, not edited."""
import math

import numpy as np

import exact_data as ed

DAMPING = 0.5
N = 2048
HUBS = [(N // 3, 1500), (N - 1, 600)]
DEGREES = [(1, 2, 4), (2, 4), (4, 8), (16, 32)]
# the floors tests/test_ppr_prover.py asserts for the seeded sets: no GPU case below is vacuous
FLOORS = {(1, 2, 4): 6, (2, 4): 6, (4, 8): 6, (16, 32): 4}
_cache = {}


def graph(degrees):
    """The 2 048-node dyadic graph of the given out-degrees: eight dangling nodes, two hub rows."""
    key = ("graph", tuple(degrees))
    if key not in _cache:
        _cache[key] = ed.dyadic_graph(np.random.default_rng(7), N, degrees, ed.DYADIC_DIRECT_DANGLING, HUBS)
    return _cache[key]


def seed_sets(n=N):
    """k = 5: an ordinary node, a dangling node, a hub, a pair, eight nodes n / 8 apart."""
    return [[17], [3], [n // 3], [17, 900], [int(i) * (n // 8) for i in range(8)]]


def teleport_matrix(n, sets):
    """V (n x k) float32: column j is 1 / |set j| on the set's nodes."""
    V = np.zeros((n, len(sets)), np.float32)
    for j, nodes in enumerate(sets):
        V[np.asarray(nodes, np.int64), j] = np.float32(1.0) / np.float32(len(nodes))
    return V


def _device_residual(diff, E):
    """(float32 the device reports, whether that is order-independent) for r_new - r_old = diff * 2^-E (float32-exact
    integers): the squares rounded to float32, summed in fp64, one square root, one rounding."""
    d = diff[diff != 0]
    if d.size == 0:
        return np.float32(0.0), True
    f = np.ldexp(d.astype(np.float64), -E).astype(np.float32)
    squares = (f * f).astype(np.float64)                   # float32 products, rounded to nearest even as __fmul_rn
    if not np.all(squares >= 2.0 ** -126):                 # no subnormal float32 square
        return np.float32(0.0), False
    mant, expo = np.frexp(squares)                         # a float32: mant * 2^24 is an integer
    ints, expo = (mant * 2.0 ** 24).astype(np.int64), expo.astype(np.int64) - 24
    low = int(expo.min())
    if int(expo.max()) - low > 1000:
        return np.float32(0.0), False
    total = sum(i << (e - low) for i, e in zip(ints.tolist(), expo.tolist()))
    # every square is a multiple of 2^low, so every partial sum is; below 2^53 of them all are exact in fp64, in any order
    if total >= 1 << 53:
        return np.float32(0.0), False
    return np.float32(np.sqrt(np.ldexp(np.float64(total), low))), True


def run(rp, ci, va, n, seeds, damping, steps):
    """The update above in int64 over a power-of-two quantum, from r_0 = v = 1 / len(seeds) on `seeds`.  Yields per step
    (ranks float32, exact residual float64, the device's residual float32, whether every operation of the step was
    exact in float32, whether the device's residual is order-independent)."""
    k = n.bit_length() - 1
    assert n == 1 << k
    seeds = np.asarray(seeds, np.int64)
    m = int(seeds.size).bit_length() - 1
    assert seeds.size == 1 << m and np.unique(seeds).size == seeds.size
    d = float(np.float32(damping)).as_integer_ratio()
    dn, dk = d[0], d[1].bit_length() - 1
    assert d[1] == 1 << dk and 0 < dn < d[1]
    mant, expo = np.frexp(np.asarray(va, np.float32))
    assert np.all(mant == 0.5)
    j = (1 - expo).astype(np.int64)
    J = int(j.max())
    rp64, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    dangling = np.bincount(ci, minlength=n) == 0
    filled = np.flatnonzero(np.diff(rp64) > 0)
    V = np.zeros(n, np.int64)                                        # v = V * 2^-m
    V[seeds] = 1
    R, e = V.copy(), m                                               # ranks = R * 2^-e
    for _ in range(steps):
        E = e + J + dk + m                                           # every quantity of the step is a multiple of 2^-E
        if E > 62:
            raise OverflowError("the step does not fit int64: not provable here")
        prod = R[ci] << (J - j)                                      # * 2^-(e + J)
        run_sum = np.concatenate([[0], np.cumsum(prod)])
        acc = run_sum[rp64[1:]] - run_sum[rp64[:-1]]
        any_bit = np.bitwise_or.reduceat(prod, rp64[filled]) if filled.size else np.zeros(0, np.int64)
        quantum = any_bit & -any_bit                                 # per row: products are multiples of it ...
        exact = bool(np.all((acc[filled] >> 24) < quantum + (any_bit == 0)))   # ... and the sum is below 2^24 of them
        s = int(R[dangling].sum())                                   # * 2^-e: the dangling mass, float(double sum)
        dacc = dn * acc                                              # * 2^-(e + J + dk)
        ds = dn * s                                                  # d * s at 2^-(e + dk)
        dsv = ds * V                                                 # (d * s) * v at 2^-(e + dk + m)
        tele = (1 << dk) - dn                                        # 1 - d at 2^-dk
        tv = tele * V                                                # (1 - d) * v at 2^-(dk + m)
        first = (dacc << m) + (dsv << J)                             # d * acc + (d * s) * v
        fresh = first + (tv << (e + J))
        diff = fresh - (R << (E - e))
        exact = exact and all(ed._fits_float32(x) for x in (s, dacc, ds, dsv, tele, tv, first, fresh, diff))
        exact = exact and int(fresh.sum()) == 1 << E                 # mass 1: the final r /= sum(r) divides by 1.0f
        square_sum = sum(int(x) * int(x) for x in diff[diff != 0])
        residual = math.ldexp(math.sqrt(square_sum), -E)
        reported, order_free = _device_residual(diff, E)
        low = int(np.bitwise_or.reduce(fresh))
        shift = (low & -low).bit_length() - 1
        R, e = fresh >> shift, E - shift
        yield np.ldexp(R.astype(np.float64), -e).astype(np.float32), residual, reported, exact, order_free


def exact_steps(rp, ci, va, n, seeds, damping, max_steps=8, with_residual=True):
    """Number of leading steps (up to max_steps) the device computes exactly; with_residual: and whose reported
    residual is order-independent."""
    count = 0
    try:
        for _, _, _, exact, order_free in run(rp, ci, va, n, seeds, damping, max_steps):
            if not exact or (with_residual and not order_free):
                break
            count += 1
    except OverflowError:
        pass
    return count


def trajectory(rp, ci, va, n, seeds, damping, steps):
    """[(ranks float32, exact residual, the device's residual float32)] after step 1, 2, ... `steps`."""
    return [(ranks, residual, reported) for ranks, residual, reported, _, _ in run(rp, ci, va, n, seeds, damping, steps)]


def proven(degrees, sets=None, n=N, graph_arrays=None, max_steps=8):
    """(steps, [trajectory per set]) on the catalogue graph of `degrees` (or graph_arrays = (rp, ci, va)): steps is
    the smallest exact_steps over the sets, every trajectory runs that long."""
    key = None
    if graph_arrays is None:
        key = ("proven", tuple(degrees), n, max_steps, None if sets is None else tuple(tuple(s) for s in sets))
    if key in _cache:
        return _cache[key]
    rp, ci, va = graph_arrays if graph_arrays is not None else graph(degrees)
    sets = seed_sets(n) if sets is None else sets
    steps = min(exact_steps(rp, ci, va, n, s, DAMPING, max_steps) for s in sets)
    out = (steps, [trajectory(rp, ci, va, n, s, DAMPING, steps) if steps else [] for s in sets])
    if key is not None:
        _cache[key] = out
    return out


# ------------------------------------------------------------------------------------------ float64 reference
def power_iteration64(rp, ci, va, n, V, damping, tolerance, max_iterations):
    """The update in float64 numpy, column by column, with the library's stop rule; returns (R n x k normalised,
    [iterations], [[residual of every step]], [converged])."""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    va64, ci = np.asarray(va, np.float64), np.asarray(ci, np.int64)
    dangling = np.bincount(ci, weights=va64, minlength=n) == 0
    d = float(np.float32(damping))
    tol = float(np.float32(tolerance))
    V = np.asarray(V, np.float64)
    out = np.empty_like(V)
    iterations, residuals, converged = [], [], []
    for j in range(V.shape[1]):
        v = V[:, j]
        r, it, history, conv = v.copy(), 0, [], False
        while it < max_iterations:
            s = r[dangling].sum()
            new = d * np.bincount(rows, weights=va64 * r[ci], minlength=n) + (d * s) * v + (1.0 - d) * v
            res = float(np.sqrt(np.sum((new - r) ** 2)))
            history.append(res)
            r = new
            it += 1
            if res < tol:
                conv = True
                break
        out[:, j] = r / r.sum()
        iterations.append(it)
        residuals.append(history)
        converged.append(conv)
    return out, iterations, residuals, converged
