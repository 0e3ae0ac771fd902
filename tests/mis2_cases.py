"""Shared helpers of tests/test_amg_mis2_host.py, tests/test_gpu_amg_setup_device.py and
tests/test_gpu_amg_mis2_trips.py: a numpy restatement of the
MIS-2 aggregation of include/spmv/amg.h, written rule for rule in amg_cases.aggregate's style; the checker of its
properties on a symmetric strong graph; the inputs, those past the grid caps included; the restated hierarchy and its
fp32 PCG; and what
tests/golden/mis2_restate.json records (tests/golden/make_mis2_golden.py writes it).  A plain module, not a
conftest."""
import importlib
import json
import os

import numpy as np

import amg_cases as ac
import exact_data as ed

spd = importlib.import_module("gpu-spmv_amd.spd")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mis2_restate.json")
SEEDS = (0, 1, 0xDEADBEEF)
THETAS = (0.0, 0.08, 0.5)
UNDECIDED, ROOT, OUT = 0, 1, 2


# ---- the rule ------------------------------------------------------------------------------------------------
def fmix32(h):
    h = np.asarray(h, np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def priorities(n, seed):
    """key[i]: a larger key comes first; the pair (fmix32(i ^ seed), i) as one integer"""
    i = np.arange(n, dtype=np.uint64)
    return (fmix32(i ^ np.uint64(seed & 0xFFFFFFFF)) << np.uint64(32)) | i


def strong_entries(n, rp, ci, va, theta):
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    va = np.asarray(va, np.float32)
    d = ac.diag32(n, rp, ci, va).astype(np.float64)
    rows = ac.rows_of(n, rp)
    th = np.float64(np.float32(theta))
    v64 = va.astype(np.float64)
    with np.errstate(all="ignore"):
        return (ci != rows) & (va != 0) & (v64 * v64 >= (th * th) * np.abs(d[rows] * d[ci]))


def neighbourhoods(n, rp, ci, strong):
    """N(i) in storage order (repeats kept) and N2(i) as a set, both from A's rows only"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    near = [ci[rp[i]:rp[i + 1]][strong[rp[i]:rp[i + 1]]] for i in range(n)]
    two = []
    for i in range(n):
        reach = set(near[i].tolist())
        for u in near[i]:
            reach.update(near[u].tolist())
        reach.discard(i)
        two.append(np.fromiter(reach, np.int64, len(reach)))
    return near, two


def aggregate(n, rp, ci, va, theta, seed):
    """amg.h's MIS-2 rule, restated; (aggregate int32[n] with -1 = free, count, synchronous rounds)"""
    return aggregate_parts(n, rp, ci, va, theta, seed)[:3]


def aggregate_parts(n, rp, ci, va, theta, seed):
    """aggregate's three results, then the root flags and `first`, the map as phase 1 leaves it (-1 = phase 2's)"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    va = np.asarray(va, np.float32)
    strong = strong_entries(n, rp, ci, va, theta)
    near, two = neighbourhoods(n, rp, ci, strong)
    key = priorities(n, seed)
    # roots: descending priority; v is a root iff no higher-priority vertex of N2(v) is one
    root = np.zeros(n, bool)
    for v in np.argsort(key)[::-1]:
        higher = two[v][key[two[v]] > key[v]]
        root[v] = not root[higher].any()
    # numbers: the roots by ascending row
    number = np.cumsum(root) - 1
    count = int(root.sum())
    # phase 1: the first root of N(i) in storage order
    first = np.where(root, number, -1)
    for i in range(n):
        if not root[i]:
            hits = near[i][root[near[i]]]
            if hits.size:
                first[i] = number[hits[0]]
    # phase 2: the largest |v| among the strong entries whose column phase 1 placed, the first on a tie
    agg = first.copy()
    for i in range(n):
        if first[i] != -1:
            continue
        best, best_abs = -1, np.float32(0)
        for p in range(rp[i], rp[i + 1]):
            if strong[p] and first[ci[p]] != -1 and (best == -1 or abs(va[p]) > best_abs):
                best, best_abs = ci[p], abs(va[p])
        if best != -1:
            agg[i] = first[best]
    # the synchronous loop
    state = np.full(n, UNDECIDED)
    rounds = 0
    higher = [two[v][key[two[v]] > key[v]] for v in range(n)]
    while (state == UNDECIDED).any():
        rounds += 1
        new = state.copy()
        for v in np.flatnonzero(state == UNDECIDED):
            seen = state[higher[v]]
            if (seen == ROOT).any():
                new[v] = OUT
            elif (seen == OUT).all():
                new[v] = ROOT
        state = new
    assert np.array_equal(state == ROOT, root)
    return agg.astype(np.int32), count, rounds, root, first


def check_properties(n, rp, ci, va, theta, agg, count, root):
    """On a symmetric strong graph, with `root` the flags of roots_of: the roots are pairwise at distance >= 3, every
    aggregate holds exactly one root, every member is within distance 2 of its root, the aggregate numbers are the
    ranks of the roots, and no vertex is left that a root does not reach (the set is maximal)."""
    strong = strong_entries(n, rp, ci, va, theta)
    near, two = neighbourhoods(n, rp, ci, strong)
    pairs = {(i, int(j)) for i in range(n) for j in near[i]}
    assert all((j, i) in pairs for i, j in pairs), "the strong graph is not symmetric"
    agg = np.asarray(agg)
    root = np.asarray(root, bool)
    ids = np.flatnonzero(root)
    assert ids.size == count and agg.min() >= 0 and agg.max() == count - 1
    assert np.array_equal(np.bincount(agg[ids], minlength=count), np.ones(count, np.int64)), "roots per aggregate"
    for r in ids:
        assert not root[two[r]].any(), ("two roots within distance 2", int(r))
    assert np.array_equal(agg[ids], np.arange(count)), "the numbers are not the ranks of the roots"
    for v in range(n):
        r = ids[agg[v]]
        assert v == r or r in two[v], ("a member further than 2 from its root", v, int(r))
    # maximality: every vertex is within distance 2 of some root
    for v in np.flatnonzero(~root):
        assert root[two[v]].any(), ("a vertex no root reaches", int(v))


def roots_of(n, rp, ci, va, theta, seed):
    strong = strong_entries(n, rp, ci, va, theta)
    _, two = neighbourhoods(n, rp, ci, strong)
    key = priorities(n, seed)
    root = np.zeros(n, bool)
    for v in np.argsort(key)[::-1]:
        higher = two[v][key[two[v]] > key[v]]
        root[v] = not root[higher].any()
    return root


# ---- inputs --------------------------------------------------------------------------------------------------
def from_dense(dense):
    dense = np.asarray(dense, np.float32)
    n = dense.shape[0]
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, cols.astype(np.int32), dense[rows, cols]


def diagonal_matrix(n):
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(1, 2, n).astype(np.float32)


def star(leaves):
    """vertex 0 joined to `leaves` leaves: a row longer than a lane group, more than 64 two-hop neighbours per leaf
    (the centre's diagonal is small enough for every edge to be strong at theta = 0.08; nothing here solves with it)"""
    n = leaves + 1
    dense = np.zeros((n, n), np.float32)
    dense[0, 1:] = dense[1:, 0] = -1.0
    np.fill_diagonal(dense, 2.0)
    dense[0, 0] = 4.0
    return from_dense(dense)


def two_grids(m):
    """two disconnected m x m grids in one matrix"""
    n, rp, ci, va = spd.poisson2d(m)
    rp2 = np.concatenate([rp, rp[1:] + rp[-1]]).astype(np.int32)
    return 2 * n, rp2, np.concatenate([ci, ci + n]).astype(np.int32), np.concatenate([va, va])


def path_equal(n):
    """tridiag(-1, 2, -1): |v| equal everywhere off the diagonal, so phase 2 decides by storage order"""
    return ac.tridiagonal(n)


def unsymmetric(n=40, seed=11):
    """random unsymmetric values AND pattern with a dominant diagonal: N2 is not symmetric"""
    rng = np.random.default_rng(seed)
    dense = np.where(rng.random((n, n)) < 0.08, rng.uniform(-1.0, -0.2, (n, n)), 0.0).astype(np.float32)
    np.fill_diagonal(dense, 4.0)
    return from_dense(dense)


SYMMETRIC = {
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
    "random_spd(500, 7, 3)": lambda: spd.random_spd(500, 7, 3),
    "random_spd(1025, 7, 5)": lambda: spd.random_spd(1025, 7, 5),
    "n = 1": lambda: diagonal_matrix(1),
    "diagonal": lambda: diagonal_matrix(37),
    "star(130)": lambda: star(130),
    "two grids": lambda: two_grids(9),
    "equal |v|": lambda: path_equal(50),
}
UNSYMMETRIC = {"unsymmetric": unsymmetric}
CASES = dict(SYMMETRIC, **UNSYMMETRIC)


# ---- inputs past the grid caps (tests/test_gpu_amg_mis2_trips.py); vectorised numpy only -------------------------
# A row kernel at L lanes covers ed.row_trip(L) rows a trip of its capped grid, an element-wise kernel ed.VEC_TRIP
# elements.  test_amg_mis2_host.py settles on the CPU what each case claims.
HUB_SPOKES = 300
TRIP_PAIRS = ((0.08, 0), (0.0, 0xDEADBEEF))            # the (theta, seed) every case past a cap is aggregated with
HUB_SEED = 5                                           # of the base matrix spd.random_spd(n, k, HUB_SEED)


def _rows_sorted(n, rows, cols, vals):
    """CSR of triplets, storage order kept inside a row (a stable sort by row)"""
    order = np.argsort(rows, kind="stable")
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, cols[order].astype(np.int32), np.asarray(vals, np.float32)[order]


def cap_hub(n, k, seed=HUB_SEED):
    """spd.random_spd(n, k, seed) (rows unsorted, columns repeated) with the last row made a hub: HUB_SPOKES spokes to
    np.linspace(0, n - 2, HUB_SPOKES), -1 both ways and stored after the base entries of their rows, every base entry
    between the hub and a spoke removed first, the hub's diagonal 4.0 (star's rule: nothing solves with it).  The hub
    row lies in the last trip of every row kernel, is longer than a lane group and gives each leaf more than 64 two-hop
    neighbours; its leaves are spread over every trip."""
    _, rp, ci, va = spd.random_spd(n, k, seed)
    rows, ci, va = ac.rows_of(n, rp), np.asarray(ci, np.int64), np.asarray(va, np.float32).copy()
    hub = n - 1
    spokes = np.unique(np.linspace(0, n - 2, HUB_SPOKES).astype(np.int64))
    assert spokes.size == HUB_SPOKES
    is_spoke = np.zeros(n, bool)
    is_spoke[spokes] = True
    keep = ~(((rows == hub) & is_spoke[ci]) | ((ci == hub) & is_spoke[rows]))
    va[(rows == hub) & (ci == hub)] = 4.0
    minus = np.full(HUB_SPOKES, -1.0, np.float32)
    return _rows_sorted(n, np.concatenate([rows[keep], np.full(HUB_SPOKES, hub), spokes]),
                        np.concatenate([ci[keep], spokes, np.full(HUB_SPOKES, hub)]),
                        np.concatenate([va[keep], minus, minus]))


def cap_unsymmetric(n, k, seed=HUB_SEED):
    """spd.random_spd(n, k, seed) with each off-diagonal entry dropped independently with probability 1/4: pattern and
    values both unsymmetric, N2 not symmetric"""
    _, rp, ci, va = spd.random_spd(n, k, seed)
    rows = ac.rows_of(n, rp)
    keep = (rows == ci) | (np.random.default_rng(seed + 1).random(ci.size) >= 0.25)
    return _rows_sorted(n, rows[keep], np.asarray(ci, np.int64)[keep], np.asarray(va, np.float32)[keep])


def priority_chain(m, seed):
    """A path with -1 off and 2 on the diagonal that visits the m vertices in descending priority under `seed`.  The
    synchronous loop decides its first vertex in round 1 and three more every two rounds: ceil(2 m / 3) rounds."""
    order = np.argsort(priorities(m, seed))[::-1].astype(np.int64)
    i = np.arange(m, dtype=np.int64)
    return _rows_sorted(m, np.concatenate([order[:-1], order[1:], i]), np.concatenate([order[1:], order[:-1], i]),
                        np.concatenate([np.full(2 * (m - 1), -1.0), np.full(m, 2.0)]).astype(np.float32))


def chain_rounds(m):
    return -(-2 * m // 3)


def _hub_k(n):
    return 7 if n <= ed.row_trip(8) else 3


# Seeds other than HUB_SEED, chosen so that the case meets test_amg_mis2_host.py's condition on its last trip: the five
# rows of the third trip at 64 lanes hold a root, a phase-1 member and a phase-2 member under both TRIP_PAIRS; the one
# row of the unsymmetric case's second trip is a root under the first pair and phase 2's under the second.
CASE_SEEDS = {("hub", 2 * ed.row_trip(64) + 5): 27, ("unsymmetric", ed.row_trip(64) + 1): 75}


def _row_cases():
    """name -> (forced mis_lanes, n, builder)"""
    cases = {}
    for L in (64, 8):
        R = ed.row_trip(L)
        for n in (R - 1, R, R + 1, 2 * R + 5):
            cases["hub L%d n=%d" % (L, n)] = (
                L, n, lambda n=n: cap_hub(n, _hub_k(n), CASE_SEEDS.get(("hub", n), HUB_SEED)))
        cases["unsymmetric L%d n=%d" % (L, R + 1)] = (
            L, R + 1, lambda n=R + 1: cap_unsymmetric(n, _hub_k(n), CASE_SEEDS.get(("unsymmetric", n), HUB_SEED)))
    for L in ed.LANES[1:]:
        if L not in (64, 8):
            n = ed.LANE_SIZES[L]
            cases["hub L%d n=%d" % (L, n)] = (L, n, lambda n=n: cap_hub(n, _hub_k(n)))
    return cases


ROW_CASES = _row_cases()
VEC_CASES = {"hub L2 n=%d" % n: (2, n, lambda n=n: cap_hub(n, 3))
             for n in (ed.VEC_TRIP - 1, ed.VEC_TRIP, ed.VEC_TRIP + 1)}
CHAIN_CASES = (12, 13, 24, 25, 40)                     # around one and two batches of kRoundsPerBatch = 8, and past two
RESTATED_ROWS = 2 * ed.row_trip(64) + 5                # up to here the restatement's Python loops are affordable


def last_trip(L, n):
    """the rows of the last trip of a row kernel at L lanes over n rows"""
    R = ed.row_trip(L)
    return np.arange((n - 1) // R * R, n)


# ---- the restated hierarchy and its PCG ------------------------------------------------------------------------
def maps(spmv, n, rp, ci, va, theta=0.08, coarse_rows=64, max_levels=10, seed=0):
    """(aggregate maps, synchronous rounds per level) of amg_setup_device's stopping rules, level by level, with the
    Galerkin products of amg_cases.galerkin (spgemm_cpu_csr on the host)"""
    out, rounds = [], []
    for l in range(max_levels - 1):
        if n <= coarse_rows:
            break
        agg, count, took = aggregate(n, rp, ci, va, theta, seed)
        if count == n:
            break
        out.append(agg)
        rounds.append(took)
        rp, ci, va = ac.galerkin(spmv, n, rp, ci, va, agg, count)
        n = count
    return out, rounds


class HostSystem:
    """what test_gpu_cg_ic.restate_ic needs: the matrix, test_gpu_bicgstab.System's right-hand side and the fp32
    V-cycle on restated levels"""

    def __init__(self, n, rp, ci, va, levels, seed=1):
        self.n, self.rp, self.ci, self.va, self.levels = n, rp, ci, va, levels
        self.b = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)

    def precondition(self, u):
        return ac.vcycle(self.levels, u, np.float32(2.0) / np.float32(3.0), 1, 1, 4, np.float32)


SOLVED = {
    "poisson2d(32)": lambda: spd.poisson2d(32),
    "poisson2d(48)": lambda: spd.poisson2d(48),
    "poisson3d(12)": lambda: spd.poisson3d(12),
}
SIZED = dict(SOLVED, **{"random_spd(500, 7, 3)": lambda: spd.random_spd(500, 7, 3)})


def restated(spmv, name, with_solve=True):
    """dict(levels = rows per level, rounds = synchronous rounds per aggregated level, steps = the fp32 restated PCG's
    step count to 1e-6, or None) of SIZED[name] at seed 0 and the default configuration"""
    from test_gpu_cg_ic import restate_ic
    n, rp, ci, va = SIZED[name]()
    given, rounds = maps(spmv, n, rp, ci, va)
    levels = ac.hierarchy(spmv, n, rp, ci, va, maps=given)
    steps = None
    if with_solve and name in SOLVED:
        _, steps, converged, breakdown, _ = restate_ic(HostSystem(n, rp, ci, va, levels), np.zeros(n), 1e-6)
        assert converged and not breakdown
    return dict(levels=[lv["n"] for lv in levels], rounds=rounds, steps=steps), given, levels


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
