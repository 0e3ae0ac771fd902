"""The MIS-2 aggregation of the device-side AMG setup (include/spmv/amg.h) on the host side (no GPU): the exported names;
amg_aggregate_mis2_cpu_csr against mis2_cases' numpy restatement, entry for entry, with its synchronous round count;
the properties of the aggregates on symmetric strong graphs; unsymmetric graphs; the tie rule; what
tests/golden/mis2_restate.json records against a fresh run; the argument checks in their order; and the sanitized
caller."""
import ctypes
import json
import os
import re
import subprocess
import time

import numpy as np
import pytest

import amg_cases as ac
import exact_data as ed
import mis2_cases as mc
from conftest import ROOT

NAMES = ("amg_aggregate_mis2_cpu_csr", "amg_aggregate_mis2_gpu", "amg_setup_device", "amg_setup_rounds")
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    cxx = open(os.path.join(ROOT, "include", "spmv", "amg.h")).read()
    for name in NAMES:
        c_name = "spmv_c_" + name
        assert c_name in declared and c_name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), c_name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert ctypes.sizeof(spmv.AMGConfig) == 28 and ctypes.sizeof(spmv.AMGResult) == 48


# ---- the aggregation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_aggregation_equals_the_restatement_entry_for_entry(spmv, name):
    n, rp, ci, va = mc.CASES[name]()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    try:
        for theta in mc.THETAS:
            for seed in mc.SEEDS:
                what = (name, theta, hex(seed))
                status, agg, count, rounds = spmv.amg_aggregate_mis2_cpu_csr(A, theta, seed)
                want, want_count, want_rounds = mc.aggregate(n, rp, ci, va, theta, seed)
                assert (status, count, rounds) == (0, want_count, want_rounds), what
                np.testing.assert_array_equal(agg, want, err_msg=str(what))
                assert 1 <= rounds <= n and agg.min() >= 0, what          # nobody is left free
                if name in mc.SYMMETRIC:
                    mc.check_properties(n, rp, ci, va, theta, agg, count, mc.roots_of(n, rp, ci, va, theta, seed))
                if name == "diagonal" or (theta == 0.5 and name.startswith(("poisson", "random", "two"))):
                    assert count == n and np.array_equal(agg, np.arange(n)), what    # all singletons, in row order
                if name == "star(130)" and theta <= 0.08:
                    assert count == 1 and (agg == 0).all(), what
        again = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
        first = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
        assert again[0] == 0 and again[2:] == first[2:] and np.array_equal(again[1], first[1])
    finally:
        spmv.csr_destroy(A)


def test_seeds_change_the_roots_and_random_spd_is_messy(spmv):
    n, rp, ci, va = mc.SYMMETRIC["random_spd(500, 7, 3)"]()
    unsorted = repeated = False
    for i in range(n):
        row = ci[rp[i]:rp[i + 1]]
        unsorted |= bool((np.diff(row) < 0).any())
        repeated |= np.unique(row).size < row.size
    assert unsorted and repeated
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    maps = [spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, seed)[1] for seed in mc.SEEDS]
    spmv.csr_destroy(A)
    assert not np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[1], maps[2])


def test_small_unsymmetric_graphs_equal_the_restatement_and_leave_nobody_free(spmv):
    """N2 is read from A's rows only, so on an unsymmetric strong graph u in N2(v) does not give v in N2(u).  A vertex
    that is not a root saw a root x either in N(v), and phase 1 places it, or in N(u) for a u in N(v), and then u is a
    root or a phase-1 member and phase 2 places v: -1 never comes out, which 60 random graphs show here."""
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(2, 13))
        dense = np.where(rng.random((n, n)) < 0.3, rng.uniform(-2.0, 2.0, (n, n)), 0.0).astype(np.float32)
        np.fill_diagonal(dense, rng.uniform(1.0, 3.0, n))
        _, rp, ci, va = mc.from_dense(dense)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        status, agg, count, rounds = spmv.amg_aggregate_mis2_cpu_csr(A, 0.25, trial)
        spmv.csr_destroy(A)
        want = mc.aggregate(n, rp, ci, va, 0.25, trial)
        assert (status, count, rounds) == (0, want[1], want[2]) and np.array_equal(agg, want[0]), trial
        assert agg.min() >= 0, trial


def test_phase_two_takes_the_largest_entry_and_the_first_on_a_tie(spmv):
    """a path 0 - 1 - 2 - 3 - 4 - 5 - 6 whose ends' neighbours are forced to be the roots by the values: vertex 3 is at
    distance 2 from both roots 1 and 5 and is placed by phase 2 through 2 or 4"""
    def matrix(left, right):
        dense = np.diag(np.full(7, 4.0, np.float32))
        for i, v in enumerate((-2.0, -2.0, left, right, -2.0, -2.0)):
            dense[i, i + 1] = dense[i + 1, i] = v
        return mc.from_dense(dense)

    found = 0
    for seed in range(200):
        n, rp, ci, va = matrix(-1.0, -1.0)
        root = mc.roots_of(n, rp, ci, va, 0.08, seed)
        if not (root[1] and root[5]):
            continue
        found += 1
        for left, right, side in ((-1.0, -1.5, 5), (-1.5, -1.0, 1), (-1.0, -1.0, 1), (1.0, -1.0, 1)):
            n, rp, ci, va = matrix(left, right)
            A = spmv.csr_from_arrays(n, n, rp, ci, va)
            status, agg, count, _ = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, seed)
            spmv.csr_destroy(A)
            assert status == 0 and count == 2 and agg[3] == agg[side], (seed, left, right, agg)
            assert agg.tolist()[:3] == [0, 0, 0] and agg.tolist()[4:] == [1, 1, 1]
            np.testing.assert_array_equal(agg, mc.aggregate(n, rp, ci, va, 0.08, seed)[0])
        if found == 3:
            break
    assert found == 3


# ---- the cases past the grid caps (tests/test_gpu_amg_mis2_trips.py) ---------------------------------------------
TRIP_CASES = dict(mc.ROW_CASES, **mc.VEC_CASES)
RESTATED = [name for name, case in TRIP_CASES.items() if case[1] <= mc.RESTATED_ROWS]


def define(spmv, n, rp, ci, va, theta, seed):
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    try:
        start = time.perf_counter()
        status, agg, count, rounds = spmv.amg_aggregate_mis2_cpu_csr(A, theta, seed)
        return status, agg, count, rounds, time.perf_counter() - start
    finally:
        spmv.csr_destroy(A)


def test_the_case_lists_are_the_caps_neighbours():
    assert len(mc.ROW_CASES) == 14 and len(mc.VEC_CASES) == 3 and len(TRIP_CASES) == 17
    sizes = {}
    for name, (L, n, _) in mc.ROW_CASES.items():
        sizes.setdefault((name.split()[0], L), []).append(n)
    for L in (64, 8):
        R = ed.row_trip(L)
        assert sizes["hub", L] == [R - 1, R, R + 1, 2 * R + 5] and sizes["unsymmetric", L] == [R + 1]
    assert ed.row_trip(64) == 8192 and ed.row_trip(2) == ed.VEC_TRIP
    for L in (2, 4, 16, 32):
        assert sizes["hub", L] == [ed.LANE_SIZES[L]] and ed.row_trip(L) < ed.LANE_SIZES[L] < 2 * ed.row_trip(L)
    assert [(L, n) for L, n, _ in mc.VEC_CASES.values()] == [(2, ed.VEC_TRIP + off) for off in (-1, 0, 1)]
    assert mc.RESTATED_ROWS == 16389 and len(RESTATED) == 5


def test_the_hub_and_the_dropped_entries_are_what_the_cases_claim():
    """cap_hub at the issue's n = 8197: a symmetric pattern with unsorted rows and repeated columns, the hub row of 316
    entries with 4.0 on its diagonal, every spoke stored once and -1 both ways, a leaf in every trip at 64 lanes;
    cap_unsymmetric: a quarter of the off-diagonal entries gone, pattern unsymmetric, the diagonal whole."""
    n, rp, ci, va = mc.cap_hub(8197, 7)
    rows, hub = ac.rows_of(n, rp), n - 1
    assert rp[n] - rp[hub] == 316
    pairs = set(zip(rows.tolist(), ci.tolist()))
    assert all((j, i) in pairs for i, j in pairs)
    spokes = np.linspace(0, n - 2, mc.HUB_SPOKES).astype(np.int64)
    hub_row, hub_vals = ci[rp[hub]:], va[rp[hub]:]
    for s in spokes:
        assert (hub_row == s).sum() == 1 and hub_vals[hub_row == s][0] == -1.0
        mine = ci[rp[s]:rp[s + 1]] == hub
        assert mine.sum() == 1 and va[rp[s]:rp[s + 1]][mine][0] == -1.0
    assert va[(rows == hub) & (ci == hub)].tolist() == [4.0]
    assert set((spokes // ed.row_trip(64)).tolist()) == {0, 1} and hub // ed.row_trip(64) == 1
    lens = np.diff(rp)
    assert any((np.diff(ci[rp[i]:rp[i + 1]]) < 0).any() for i in range(200))
    assert any(np.unique(ci[rp[i]:rp[i + 1]]).size < lens[i] for i in range(n))
    _, base_rp, base_ci, _ = mc.spd.random_spd(8197, 7, mc.HUB_SEED)
    n, rp, ci, va = mc.cap_unsymmetric(8197, 7)
    rows = ac.rows_of(n, rp)
    dropped = (base_ci.size - ci.size) / (base_ci.size - n)
    assert 0.23 < dropped < 0.27 and (rows == ci).sum() == n
    pairs = set(zip(rows.tolist(), ci.tolist()))
    assert sum((j, i) not in pairs for i, j in pairs) > 1000


def test_the_numbers_the_cases_were_designed_on(spmv):
    """n = 8197 = exact_data.LANE_SIZES[64], k = 7, seed 5, under both TRIP_PAIRS: (aggregates, synchronous rounds)"""
    for build, want in ((mc.cap_hub, [(997, 15), (202, 15)]), (mc.cap_unsymmetric, [(1524, 10), (348, 12)])):
        got = []
        for theta, seed in mc.TRIP_PAIRS:
            status, agg, count, rounds, _ = define(spmv, *build(8197, 7), theta, seed)
            assert status == 0 and agg.min() >= 0
            got.append((count, rounds))
        assert got == want, (build.__name__, got)


@pytest.mark.parametrize("name", list(TRIP_CASES))
def test_the_definition_leaves_nobody_free_past_the_caps(spmv, name):
    """what the device test relies on: status 0, no -1, 1 < count < n, in a time a GPU test can afford (printed)"""
    L, n, build = TRIP_CASES[name]
    matrix = build()
    assert matrix[0] == n
    for theta, seed in mc.TRIP_PAIRS:
        status, agg, count, rounds, took = define(spmv, *matrix, theta, seed)
        print(f"{name} theta={theta} seed={seed:#x}: {count} aggregates, {rounds} rounds, {took:.2f} s")
        assert status == 0 and agg.min() >= 0 and agg.max() == count - 1 and 1 < count < n, (name, theta, seed, count)
        assert 1 <= rounds <= n


def kinds_of(root, first, rows):
    """(roots, phase-1 members, phase-2 members) among `rows`"""
    return (int(root[rows].sum()), int((~root[rows] & (first[rows] != -1)).sum()), int((first[rows] == -1).sum()))


@pytest.mark.parametrize("name", RESTATED)
def test_restatement_and_last_trip_of_the_cases_up_to_three_trips_at_64_lanes(spmv, name):
    """The restatement equals the definition entry for entry, and the rows of the LAST trip of the row kernels hold a
    root, a phase-1 member and a phase-2 member (first == -1 before phase 2) under both TRIP_PAIRS, so that a last
    trip that is dropped, or reads stale states, changes ints of every kind.  A last trip of ONE row (n = R_64 + 1)
    cannot hold three kinds: there the hub case's row, the hub itself, is a phase-1 member under both pairs, and the
    unsymmetric case's seed makes its row a root under the first pair and phase 2's under the second."""
    L, n, build = TRIP_CASES[name]
    matrix = build()
    rows = mc.last_trip(L, n)
    assert rows[-1] == n - 1 and rows.size == (n - 1) % ed.row_trip(L) + 1
    found = []
    for theta, seed in mc.TRIP_PAIRS:
        status, agg, count, rounds, _ = define(spmv, *matrix, theta, seed)
        want, want_count, want_rounds, root, first = mc.aggregate_parts(*matrix, theta, seed)
        assert (status, count, rounds) == (0, want_count, want_rounds), (name, theta, seed)
        np.testing.assert_array_equal(agg, want, err_msg=str((name, theta, seed)))
        found.append(kinds_of(root, first, rows))
    print(name, "roots, phase-1 and phase-2 members in the last trip of", rows.size, "rows:", found)
    if rows.size > 1:
        assert all(min(k) >= 1 for k in found), (name, found)
    elif name.startswith("hub"):
        assert found == [(0, 1, 0), (0, 1, 0)], (name, found)
    else:
        assert found == [(1, 0, 0), (0, 0, 1)], (name, found)
    if name.startswith("hub"):
        _, rp, _, _ = matrix
        assert n - 1 in rows and rp[n] - rp[n - 1] > 64


@pytest.mark.parametrize("m", mc.CHAIN_CASES + (26,))
def test_priority_chains_take_two_rounds_per_three_vertices(spmv, m):
    want = {12: 8, 13: 9, 24: 16, 25: 17, 26: 18, 40: 27}[m]
    assert mc.chain_rounds(m) == want
    for seed in (0, 1, 0xDEADBEEF):
        n, rp, ci, va = mc.priority_chain(m, seed)
        assert n == m and rp[m] == 3 * m - 2 and sorted(np.diff(rp).tolist()) == [2, 2] + [3] * (m - 2)
        status, agg, count, rounds, _ = define(spmv, n, rp, ci, va, 0.08, seed)
        restated = mc.aggregate(n, rp, ci, va, 0.08, seed)
        assert (status, rounds, restated[2]) == (0, want, want), (m, seed, rounds, restated[2])
        assert count == restated[1] == -(-m // 3) and np.array_equal(agg, restated[0]) and agg.min() >= 0
    # another seed's priorities do not walk the path in order: the chain is the slow case, not the usual one
    n, rp, ci, va = mc.priority_chain(m, 0)
    assert define(spmv, n, rp, ci, va, 0.08, 1)[3] < want


# ---- the golden ----------------------------------------------------------------------------------------------
def test_golden_levels_rounds_and_steps_against_a_fresh_run(spmv):
    golden = mc.golden()
    assert sorted(golden) == sorted(mc.SIZED)
    for name in mc.SIZED:
        fresh, given, levels = mc.restated(spmv, name)
        assert json.loads(json.dumps(fresh)) == golden[name], (name, fresh, golden[name])
        # the restated maps are the library's, level by level
        for level, want in zip(levels, given):
            A = spmv.csr_from_arrays(level["n"], level["n"], level["rp"], level["ci"], level["va"])
            status, agg, count, _ = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
            spmv.csr_destroy(A)
            assert status == 0 and count == level["count"] and np.array_equal(agg, want), name
    # the design prototype's sizes (a cross-check of the restatement, not constants the library is held to)
    assert golden["poisson2d(32)"]["levels"] == [1024, 150, 22] and golden["poisson3d(12)"]["levels"] == [1728, 172, 21]
    assert golden["poisson2d(48)"]["levels"] == [2304, 334, 48] and golden["random_spd(500, 7, 3)"]["levels"] == [500, 61]


# ---- rejections ------------------------------------------------------------------------------------------------
def test_aggregate_checks_in_the_stated_order_with_nothing_written(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    f32 = lambda v: np.asarray(v, np.float32)
    A = spmv.csr_from_arrays(3, 3, [0, 2, 3, 5], [0, 1, 1, 1, 2], f32([2, -1, 2, -1, 2]))
    R = spmv.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], f32([1, 1]))
    agg = np.full(3, -7, np.int32)
    count, rounds = ctypes.c_int32(-7), ctypes.c_int32(-7)
    ptr = agg.ctypes.data_as(ctypes.c_void_p)
    call = lib.spmv_c_amg_aggregate_mis2_cpu_csr
    assert call(None, 0.08, 0, ptr, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_ARGUMENT
    assert call(A, 0.08, 0, None, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_ARGUMENT
    assert call(A, 0.08, 0, ptr, None, ctypes.byref(rounds)) == E.INVALID_ARGUMENT
    assert call(R, -1.0, 0, ptr, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_DIMENSION
    for rp, ci in (([0, 2, 3, 4], [0, 1, 1, 1, 2]), ([1, 2, 3, 5], [0, 1, 1, 1, 2]), ([0, 3, 2, 5], [0, 1, 1, 1, 2]),
                   ([0, 2, 3, 5], [0, 1, 1, 3, 2]), ([0, 2, 3, 5], [0, -1, 1, 1, 2])):
        X = spmv.csr_from_arrays(3, 3, rp, ci, f32([2, -1, 2, -1, 2]))
        assert call(X, -1.0, 0, ptr, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_FORMAT, (rp, ci)
        spmv.csr_destroy(X)
    D = spmv.csr_wrap_device(3, 3, 5, FAKE_RP, FAKE_CI, FAKE_VA)                 # no host arrays
    assert call(D, 0.08, 0, ptr, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_FORMAT
    for theta in (-0.5, float("nan")):
        assert call(A, theta, 0, ptr, ctypes.byref(count), ctypes.byref(rounds)) == E.INVALID_ARGUMENT
    assert count.value == -7 and rounds.value == -7 and (agg == -7).all()
    assert call(A, 0.08, 0, ptr, ctypes.byref(count), None) == 0 and count.value >= 1      # rounds may be null
    for M in (A, R, D):
        spmv.csr_destroy(M)


def test_device_calls_reject_before_any_device_work(spmv):
    """fake device addresses that must never be dereferenced"""
    E = spmv.SpMVError
    A = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    R = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    Z = spmv.csr_wrap_device(0, 0, 0, FAKE_RP, None, None)
    H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], np.ones(2, np.float32))    # host only
    NC = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
    lib = spmv.lib()
    out = spmv.AMGResult(error_code=7, levels=9)
    assert lib.spmv_c_amg_setup_device(None, A, None, 0, ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and (out.levels, out.bad_row, out.bad_level) == (0, -1, -1)
    handle = ctypes.c_void_p(0x1234)
    assert lib.spmv_c_amg_setup_device(ctypes.byref(handle), None, None, 0, None) == E.INVALID_ARGUMENT
    assert handle.value is None                                                  # *out is null on failure
    bad_cfg = spmv.AMGConfig(max_levels=0)
    for M, code in ((R, E.INVALID_DIMENSION), (Z, E.INVALID_DIMENSION), (H, E.INVALID_FORMAT), (NC, E.INVALID_FORMAT)):
        res, handle = spmv.amg_setup_device(M, bad_cfg)
        assert res.error_code == code and handle is None
    for field, value in (("max_levels", 0), ("coarse_rows", 0), ("coarse_rows", 1025), ("strength", -0.1),
                         ("strength", float("nan")), ("pre_sweeps", 0), ("post_sweeps", -1), ("jacobi_weight", 0.0),
                         ("jacobi_weight", 2.0), ("jacobi_weight", float("nan")), ("coarse_sweeps", 0)):
        res, handle = spmv.amg_setup_device(A, spmv.AMGConfig(**{field: value}))
        assert res.error_code == E.INVALID_ARGUMENT and handle is None, (field, value)
    # the single-level device call
    count = ctypes.c_int32(-7)
    call = lib.spmv_c_amg_aggregate_mis2_gpu
    assert call(None, 0.08, 0, 0x1000, ctypes.byref(count), None) == E.INVALID_ARGUMENT
    assert call(A, 0.08, 0, None, ctypes.byref(count), None) == E.INVALID_ARGUMENT
    assert call(A, 0.08, 0, 0x1000, None, None) == E.INVALID_ARGUMENT
    assert call(R, -1.0, 0, 0x1000, ctypes.byref(count), None) == E.INVALID_DIMENSION
    assert call(H, -1.0, 0, 0x1000, ctypes.byref(count), None) == E.INVALID_FORMAT
    assert call(NC, -1.0, 0, 0x1000, ctypes.byref(count), None) == E.INVALID_FORMAT
    for theta in (-0.5, float("nan")):
        assert call(A, theta, 0, 0x1000, ctypes.byref(count), None) == E.INVALID_ARGUMENT
    assert count.value == -7
    assert spmv.amg_setup_rounds(None, 0) == 0
    for M in (A, R, Z, H, NC):
        spmv.csr_destroy(M)


# ---- the sanitized caller --------------------------------------------------------------------------------------
def test_amg_mis2_host_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-amg-mis2 builds tests/cpp/bin/amg_mis2_host_sanitized (csrc/amg_mis2_host.cpp and
    tests/cpp/amg_mis2_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-amg-mis2"],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "amg_mis2_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
