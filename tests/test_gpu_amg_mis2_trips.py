"""The device-side AMG setup (csrc/amg_setup.hip) past its grid caps, every comparison at zero
tolerance: the ints of amg_aggregate_mis2_cpu_csr, the definition; bits of values; ints of structure.

R_L = 524 288 / L rows a trip of a row kernel at L lanes (8192 at 64), V = 262 144 elements a trip of an element-wise
kernel (exact_data.row_trip, VEC_TRIP).  tests/test_amg_mis2_host.py settles on the CPU what each case of
mis2_cases.ROW_CASES / VEC_CASES / CHAIN_CASES claims; nothing here is measured first and asserted afterwards.

kernel                                   case that gives it a second trip                       rows in the last trip
mis2_round_, mis2_phase1_,               "hub L64": n = R_64 - 1, R_64 (one trip, 2048 full      all; all; 1 (the hub row,
mis2_phase2_kernel<64>                   workgroups), R_64 + 1, 2 R_64 + 5 (the third trip)      316 entries); 5
the same three at 8 lanes                "hub L8": R_8 - 1, R_8, R_8 + 1, 2 R_8 + 5              all; all; 1; 5
the same three at 2, 4, 16, 32 lanes     "hub L": n = R_L + 256 / L + 1                          129; 65; 17; 9
the same at 64 and 8 lanes, N2 not       "unsymmetric": n = R_64 + 1, R_8 + 1                    1
symmetric
mis2_init_, mis2_flags_kernel, the scan, VEC_CASES at 2 lanes (R_2 = V): n = V - 1, V, V + 1     none; rank[V] alone; row V
amg_diag_kernel (d), row kernels <2>                                                             and rank[V], rank[V + 1]
amg_prolongation_kernel, and all of the  amg_setup_device on cap_hub(V, 3): p_rp[V] alone;       1
above at the library's own lanes         level 1 at the lanes the library picks (printed)
amg_diag_kernel (wd, the bad row),       tridiag of V + 600 rows: 1024 partials, three           600
min_fold_kernel                          workgroups with a second trip
mis2_round_kernel's remaining[3] over    priority_chain(m): ceil(2 m / 3) synchronous rounds,    -
run_rounds' batches of 8                 m = 12, 13, 24, 25, 40 -> 8, 9, 16, 17, 27

rank[n] is the one element whose write no result shows: the scan is exclusive, so its last output, the count, is the
sum of rank[0 .. n) whatever rank[n] held (mis2_flags_kernel bounded to i < n passes every test here, at n = V too).
amg_diag_kernel's minimum needs a bad row in the FIRST trip of a thread whose second trip is good (row 44 below): a
kernel that keeps only its last trip's minimum passes the other four sets.

In cap_hub the hub row n - 1 always lies in the last trip; its 300 leaves are spread over every trip, so the in-place
state updates of one launch are read across trips and workgroups.  The device decides in place and may take fewer
rounds than the synchronous loop, never more (Level.check asserts 1 <= rounds <= the definition's); the chains print
what it took."""
import importlib

import numpy as np
import pytest

import amg_cases as ac
import array_views
import exact_data as ed
import mis2_cases as mc
import precond_trip_cases as pt

pytestmark = pytest.mark.gpu

device_tests = importlib.import_module("test_gpu_amg_setup_device")
Level, DeviceHier, on_device = device_tests.Level, device_tests.DeviceHier, device_tests.on_device
definition_maps = device_tests.definition_maps
amg_tests = importlib.import_module("test_gpu_amg")
Hier, assert_levels_equal = amg_tests.Hier, amg_tests.assert_levels_equal
bits = ac.bits
V = ed.VEC_TRIP


TRIP_CASES = dict(mc.ROW_CASES, **mc.VEC_CASES)
PAIRS = range(len(mc.TRIP_PAIRS))
_matrices, _wanted = {}, {}


@pytest.fixture(scope="module", autouse=True)
def shared_references():
    """the matrices and the definition's ints, made once per case and pair and shared by the tests below"""
    yield
    _matrices.clear()
    _wanted.clear()


def matrix_of(name):
    if name not in _matrices:
        _matrices[name] = TRIP_CASES[name][2]()
    return _matrices[name]


def wanted(gpu, name, pair):
    """(aggregate map, count, synchronous rounds) of amg_aggregate_mis2_cpu_csr for mc.TRIP_PAIRS[pair]"""
    if (name, pair) not in _wanted:
        n, rp, ci, va = matrix_of(name)
        A = gpu.csr_from_arrays(n, n, rp, ci, va)
        status, agg, count, rounds = gpu.amg_aggregate_mis2_cpu_csr(A, *mc.TRIP_PAIRS[pair])
        gpu.csr_destroy(A)
        assert status == 0 and agg.min() >= 0 and 1 < count < n, (name, pair, status, count)   # nobody free
        agg.setflags(write=False)
        _wanted[name, pair] = (agg, count, rounds)
    return _wanted[name, pair]


def compare_case(gpu, monkeypatch, name, pair):
    """Level.check (the output poisoned, the map entry for entry, the count, 1 <= rounds <= the definition's) at the
    case's forced lane count"""
    lanes = TRIP_CASES[name][0]
    theta, seed = mc.TRIP_PAIRS[pair]
    level = Level(gpu, *matrix_of(name))
    try:
        level.expected[theta, seed] = wanted(gpu, name, pair)
        monkeypatch.setenv("SPMV_DEBUG", f"mis_lanes={lanes}")
        level.check(theta, seed, what=(name, lanes))
    finally:
        level.close()


# ------------------------------------------------------------------------------------------ a. the row kernels
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("name", list(mc.ROW_CASES))
def test_every_row_kernel_past_its_cap(gpu, monkeypatch, name, pair):
    compare_case(gpu, monkeypatch, name, pair)


# ------------------------------------------------------------------------------------------ b. n + 1 elements
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("name", list(mc.VEC_CASES))
def test_the_n_plus_one_element_kernels_at_the_vector_cap(gpu, monkeypatch, name, pair):
    """below, at and just past the cap of the row kernels at 2 lanes and of the element-wise kernels: at V + 1 the second
    trip of every kernel of the level is row V alone (and rank[V + 1]); at V that of mis2_flags_kernel is rank[V]"""
    compare_case(gpu, monkeypatch, name, pair)


# ------------------------------------------------------------------------------------------ c. the round batches
@pytest.mark.parametrize("lanes", (1, 64))
@pytest.mark.parametrize("m", mc.CHAIN_CASES)
def test_chains_across_the_round_batches(gpu, monkeypatch, m, lanes):
    """No lower bound on the device's rounds: deciding in place may legally take a chain faster."""
    monkeypatch.setenv("SPMV_DEBUG", f"mis_lanes={lanes}")
    for seed in (0, 0xDEADBEEF):
        level = Level(gpu, *mc.priority_chain(m, seed))
        try:
            want, count, rounds = level.want(0.08, seed)
            assert rounds == mc.chain_rounds(m), (m, seed, rounds)
            level.check(0.08, seed, what=("chain", m, lanes))
            status, got_count, got_rounds = gpu.amg_aggregate_mis2_gpu(level.A, level.d_agg, 0.08, seed)
            assert status == 0 and got_count == count and 1 <= got_rounds <= mc.chain_rounds(m)
            print(f"priority_chain({m}, {seed:#x}) at mis_lanes={lanes}: {got_rounds} rounds on the device, "
                  f"{rounds} synchronous")
        finally:
            level.close()


# ------------------------------------------------------------------------------------------ d. the whole setup
def test_device_setup_at_the_vector_cap(gpu):
    """amg_setup_device on cap_hub(V, 3), three levels, against amg_setup handed the definition's maps: every level
    bit for bit, the rounds, and the bits of one amg_apply.  amg_prolongation_kernel's second trip is p_rp[V] alone."""
    name = "hub L2 n=%d" % V
    n, rp, ci, va = matrix_of(name)
    cfg = gpu.AMGConfig(max_levels=3)
    assert (cfg.strength, 0) == tuple(np.float32(v) for v in mc.TRIP_PAIRS[0])
    first, count, took = wanted(gpu, name, 0)              # level 0's map: case b's reference, not made again
    coarse = ac.galerkin(gpu, n, rp, ci, va, first, count)
    more, more_rounds = definition_maps(gpu, count, *coarse, gpu.AMGConfig(max_levels=2), 0)
    maps, rounds = [first] + more, [took] + more_rounds
    assert len(maps) == 2 and count > ed.row_trip(64)
    dev = DeviceHier(gpu, n, rp, ci, va, cfg, 0)
    host = Hier(gpu, n, rp, ci, va, cfg, maps)
    try:
        assert dev.res.error_code == 0 and dev.H is not None and (dev.res.bad_row, dev.res.bad_level) == (-1, -1)
        assert host.res.error_code == 0
        assert (dev.res.levels, dev.res.coarse_solver) == (host.res.levels, host.res.coarse_solver)
        assert dev.res.levels == 3
        views = [gpu.amg_level(dev.H, l)[1] for l in range(3)]
        print("rows, entries and the lanes the library picks per level:",
              [(v.num_rows, v.nnz, ed.lanes_for(v.nnz, v.num_rows)) for v in views])
        assert_levels_equal(dev.levels(), host.levels(), "cap_hub(V, 3)")
        for l, took in enumerate(rounds):
            assert 1 <= gpu.amg_setup_rounds(dev.H, l) <= took, (l, took)
        r = np.random.default_rng(11).uniform(-1, 1, n).astype(np.float32)
        z = dev.apply(r)
        assert np.isfinite(z).all()
        np.testing.assert_array_equal(bits(z), bits(host.apply(r)))
    finally:
        dev.close()
        host.close()


# ------------------------------------------------------------------------------------------ e. the diagonal
BAD_ROWS = V + 600
NO_DIAGONAL = "no diagonal"
# (rows, their bad values); the smallest row is the one reported.  amg_diag_kernel runs 1024 workgroups here, of
# which 0, 1 and 2 take a second trip: V + 300 is thread 44 of workgroup 1's second trip, 256 * 700 + 3 lies in
# workgroup 700 (past min_fold_kernel's first 256 partials), V - 1 in the last workgroup, V + 5 in workgroup 0's second
# trip, and 44 is the FIRST trip of a thread whose second trip (row V + 44) is good.
BAD_SETS = (
    ((BAD_ROWS - 1,), (0.0,)),
    ((V + 300, 256 * 700 + 3), (-4.0, np.nan)),
    ((V - 1,), (np.inf,)),
    ((V + 300, V + 5), (NO_DIAGONAL, -4.0)),
    ((V + 300, 44), (0.0, NO_DIAGONAL)),
)


def with_bad_rows(n, rp, ci, va, rows, values):
    va = va.copy()
    keep = np.ones(ci.size, bool)
    owner = ac.rows_of(n, rp)
    for row, value in zip(rows, values):
        at = np.flatnonzero((owner == row) & (ci == row))
        assert at.size == 1
        if value == NO_DIAGONAL:
            keep[at] = False
        else:
            va[at] = value
    rp2 = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(owner[keep], minlength=n), out=rp2[1:])
    return n, rp2, ci[keep], va[keep]


def test_the_smallest_bad_row_across_trips_and_partials(gpu):
    """amg_diag_kernel's minimum across trips and workgroups and min_fold_kernel over 1024 partials, with one level
    (the diagonal kernel and the fold alone) and at the default max_levels (the check rides along with one
    aggregation); then amg_update on the one-level hierarchy.  One level of more than 1024 rows is Jacobi-solved:
    with coarse_sweeps = 1 amg.h's cycle is z_i = wd_i r_i, wd_i = float(double(omega) / double(d_i)), exact for
    omega = 1/2, d_i a power of two and integer r.  wd in rows >= V is written by amg_diag_kernel's second trip
    alone."""
    E = gpu.SpMVError
    n, rp, ci, va = pt.tridiagonal(BAD_ROWS)
    one_level = gpu.AMGConfig(max_levels=1, jacobi_weight=0.5, coarse_sweeps=1)
    for rows, values in BAD_SETS:
        bad = with_bad_rows(n, rp, ci, va, rows, values)
        for cfg in (one_level, None):
            h = DeviceHier(gpu, *bad, cfg)
            try:
                assert h.H is None, (rows, cfg is None)
                assert (h.res.error_code, h.res.bad_level, h.res.bad_row) == (E.INVALID_ARGUMENT, 0, min(rows)), \
                    (rows, values, cfg is None, h.res.error_code, h.res.bad_level, h.res.bad_row)
            finally:
                h.close()
    # a good one-level setup, a bad update, a good update with other diagonals, one cycle
    owner = ac.rows_of(n, rp)
    r = ac.exact_rhs(n)
    h = DeviceHier(gpu, n, rp, ci, va, one_level)
    try:
        assert (h.res.error_code, h.res.levels, h.res.coarse_solver) == (0, 1, 1)
        np.testing.assert_array_equal(bits(h.apply(r)), bits(r * np.float32(0.25)))          # wd = (1/2) / 2
        B = on_device(gpu, *with_bad_rows(n, rp, ci, va, (V + 300,), (-4.0,)))
        res = gpu.amg_update(h.H, B)
        assert (res.error_code, res.bad_level, res.bad_row) == (E.INVALID_ARGUMENT, 0, V + 300)
        powers = np.ldexp(np.float32(1.0), 1 + (np.arange(n) * 7 + np.arange(n) // V) % 5).astype(np.float32)
        fresh = np.where(ci == owner, powers[owner], va).astype(np.float32)
        G = on_device(gpu, n, rp, ci, fresh)
        res = gpu.amg_update(h.H, G)
        assert (res.error_code, res.levels, res.coarse_solver, res.bad_row) == (0, 1, 1, -1)
        level = dict(n=n, rp=rp, ci=ci, va=fresh, agg=None, count=0)
        want = ac.vcycle([level], r, 0.5, 1, 1, 1, np.float32)
        np.testing.assert_array_equal(bits(want), bits(r * (np.float32(0.5) / powers)))       # the header's z_i = wd_i r_i
        got = h.apply(r)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
        gpu.csr_destroy(B)
        gpu.csr_destroy(G)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------ f. views
def test_the_last_trip_writes_nothing_past_the_map(gpu, monkeypatch):
    """the three-trip case at 64 lanes on arrays that are views into larger buffers: the ints, and every guard word"""
    name = "hub L64 n=%d" % (2 * ed.row_trip(64) + 5)
    lanes = mc.ROW_CASES[name][0]
    n, rp, ci, va = matrix_of(name)
    monkeypatch.setenv("SPMV_DEBUG", f"mis_lanes={lanes}")
    for pair, offsets in zip(PAIRS, ((1, 2, 3, 1), (3, 0, 1, 2))):
        theta, seed = mc.TRIP_PAIRS[pair]
        want, count, _ = wanted(gpu, name, pair)
        with array_views.Views(gpu) as views:
            A, _ = views.csr(n, n, rp, ci, va, offsets[:3])
            out = views.out(n, offsets[3])
            status, got_count, _ = gpu.amg_aggregate_mis2_gpu(A, out.ptr, theta, seed)
            assert status == 0 and got_count == count
            assert np.array_equal(out.download().view(np.int32), want), (name, offsets)
            views.check_guards("amg_aggregate_mis2_gpu past the cap")
