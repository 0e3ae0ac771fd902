"""The smoothed-aggregation part of include/spmv/amg.h on the host side (no GPU): the exported names and the layout of
AMGSmoothing; amg_prolongator_cpu_csr against the restated chain of host twins, entry for entry, and against
Fractions where the smoothed prolongator is 3/4 and 1/4; every check that needs no device, with fake device addresses
that must never be dereferenced; the transfer prover's verdicts on the cases the GPU tests run; the exact family of
tests/test_gpu_amg_smoothed_trips.py (precond_trip_cases.SMOOTHED_CASES: the caps each case passes, the coarse
diagonal of 1/2, the vectorised cycle prover against its Fraction twin and against both numpy cycles); and the
sanitized caller."""
import ctypes
import importlib
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import amg_cases as ac
import amg_smoothed_cases as sc
import exact_data as ed
import precond_trip_cases as pt
from amg_cases import bits
from exact_data import VEC_TRIP, row_trip
from conftest import ROOT

spd = importlib.import_module("gpu-spmv_amd.spd")

NAMES = ("amg_setup_smoothed", "amg_setup_smoothed_device", "amg_is_smoothed", "amg_level_transfer",
         "amg_prolongator_cpu_csr", "amg_restrict", "amg_prolong")
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def test_names_in_the_header_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    cxx = open(os.path.join(ROOT, "include", "spmv", "amg.h")).read()
    for name in NAMES:
        c_name = "spmv_c_" + name
        assert c_name in declared and c_name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), c_name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name


def test_struct_layout_and_defaults(spmv):
    S = spmv.AMGSmoothing
    assert ctypes.sizeof(S) == 8 and [getattr(S, f).offset for f, _ in S._fields_] == [0, 4]
    s = S()
    assert s.prolongator_weight == np.float32(2.0) / np.float32(3.0) and s.strength_decay == np.float32(0.5)
    # the two older structs keep their layouts
    assert ctypes.sizeof(spmv.AMGConfig) == 28 and ctypes.sizeof(spmv.AMGResult) == 48


# ---- the prolongator --------------------------------------------------------------------------------------------
def prolongator_cases():
    n, rp, ci, va = ac.tridiagonal(64)
    yield "tridiagonal(64), pairs", (n, rp, ci, va), ac.pair_maps(64, 32)[0], 32, 2.0 / 3.0
    for name, make in (("poisson2d(8)", lambda: spd.poisson2d(8)), ("random_spd(200, 7, 3)", lambda: spd.random_spd(200, 7, 3))):
        n, rp, ci, va = make()
        agg, count = ac.aggregate(n, rp, ci, va, 0.08)
        yield name, (n, rp, ci, va), agg, count, 2.0 / 3.0
        yield name + ", omega_p = 1.25", (n, rp, ci, va), agg, count, 1.25


def test_prolongator_equals_the_restated_chain_entry_for_entry(spmv):
    for name, (n, rp, ci, va), agg, count, weight in prolongator_cases():
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        P = spmv.csr_create(0, 0, 0)
        try:
            assert spmv.amg_prolongator_cpu_csr(P, A, agg, count, weight) == 0, name
            assert (P.contents.num_rows, P.contents.num_cols) == (n, count), name
            got = spmv.csr_host_arrays(P)
            want = sc.prolongator(spmv, n, rp, ci, va, agg, count, weight)
            np.testing.assert_array_equal(got[0], want[0], err_msg=name)
            np.testing.assert_array_equal(got[1], want[1], err_msg=name)
            np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg=name)
            # AT's pattern: ascending columns, and column agg_i stored in every row
            for i in range(n):
                row = got[1][got[0][i]:got[0][i + 1]]
                assert (np.diff(row) > 0).all() and agg[i] in row, (name, i)
            assert np.isfinite(got[2]).all()
        finally:
            spmv.csr_destroy(A)
            spmv.csr_destroy(P)


def test_random_spd_200_has_unsorted_rows_and_repeated_columns():
    n, rp, ci, va = spd.random_spd(200, 7, 3)
    unsorted = repeated = False
    for i in range(n):
        row = ci[rp[i]:rp[i + 1]]
        unsorted |= bool((np.diff(row) < 0).any())
        repeated |= np.unique(row).size < row.size
    assert unsorted and repeated


def test_half_weight_on_the_tridiagonal_matrix_is_three_quarters_and_one_quarter(spmv):
    """tridiag(-1, 2, -1), pairs {2a, 2a+1}, omega_p = 1/2: s = -1/4, row 2a of A T is (-1, 1) at columns a-1, a and row
    2a+1 is (1, -1) at a, a+1, so P holds 1 - 1/4 = 3/4 in the row's own aggregate and 1/4 beside it."""
    n, rp, ci, va = ac.tridiagonal(64)
    agg = ac.pair_maps(64, 32)[0]
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    P = spmv.csr_create(0, 0, 0)
    try:
        assert spmv.amg_prolongator_cpu_csr(P, A, agg, 32, 0.5) == 0
        prp, pci, pva = spmv.csr_host_arrays(P)
        for i in range(n):
            a = i // 2
            beside = a - 1 if i % 2 == 0 else a + 1
            want = {a: Fraction(3, 4)}
            if 0 <= beside < 32:
                want[beside] = Fraction(1, 4)
            got = {int(pci[p]): Fraction(float(pva[p])) for p in range(prp[i], prp[i + 1])}
            assert got == want, (i, got, want)
    finally:
        spmv.csr_destroy(A)
        spmv.csr_destroy(P)


# ---- the prover -------------------------------------------------------------------------------------------------
def transfer_levels(spmv):
    """name -> level 0 of the three exact cases of tests/test_gpu_amg_smoothed.py"""
    n, rp, ci, va = ac.tridiagonal(1040)
    yield "tridiagonal(1040), blocks of 260", sc.hierarchy(spmv, n, rp, ci, va, maps=[sc.block_map(1040, 260)], weight=0.5)[0]
    n, rp, ci, va = sc.arrow(300)
    yield "arrow(300), singletons", sc.hierarchy(spmv, n, rp, ci, va, maps=[np.arange(300, dtype=np.int32)], weight=0.5)[0]
    n, rp, ci, va = ac.tridiagonal(64)
    yield "tridiagonal(64), pairs", sc.hierarchy(spmv, n, rp, ci, va, maps=ac.pair_maps(64, 32), weight=0.5)[0]


def test_the_prover_admits_the_three_transfer_cases_and_rejects_others(spmv):
    shapes = {}
    for name, level in transfer_levels(spmv):
        f, x, e = sc.exact_vectors(level)
        fc, out, width = sc.prove_transfers(level, f, x, e)
        assert fc is not None and width <= 24, (name, width)
        assert fc.shape == (level["count"],) and out.shape == (level["n"],)
        shapes[name] = (int(np.diff(level["P"][0]).max()), int(np.diff(level["PT"][0]).max()))
        # the exact answers are what fp64 numpy gives
        res = f.astype(np.float64) - ac._spmv(level, x.astype(np.float64), np.float64)
        np.testing.assert_array_equal(fc.astype(np.float64), sc._matvec(level["count"], level["PT"], res, np.float64))
        np.testing.assert_array_equal(out.astype(np.float64),
                                      x + sc._matvec(level["n"], level["P"], e.astype(np.float64), np.float64))
    # the row lengths the lane tests rely on: 262 = 256 + 6 entries, and rows of 300
    assert shapes == {"tridiagonal(1040), blocks of 260": (2, 262), "arrow(300), singletons": (300, 300),
                      "tridiagonal(64), pairs": (2, 4)}, shapes
    # vectors too large for 24 bits, and a weight whose s is not a short dyadic number
    name, level = next(transfer_levels(spmv))
    f, x, e = sc.exact_vectors(level)
    fc, _, why = sc.prove_transfers(level, f * np.float32(1 << 22), x, e)
    assert fc is None and "bits" in why
    n, rp, ci, va = ac.tridiagonal(64)
    level = sc.hierarchy(spmv, n, rp, ci, va, maps=ac.pair_maps(64, 32), weight=2.0 / 3.0)[0]
    fc, _, why = sc.prove_transfers(level, *sc.exact_vectors(level))
    assert fc is None and "bits" in why


def test_theta_decays_per_level_in_the_restatement(spmv):
    """theta_l = fl32(theta_{l-1} * decay), and on poisson3d(8) the decay changes the level sizes: without it the
    second aggregation of the denser smoothed operator stalls"""
    n, rp, ci, va = spd.poisson3d(8)
    halved = sc.hierarchy(spmv, n, rp, ci, va, coarse_rows=8)
    fixed = sc.hierarchy(spmv, n, rp, ci, va, coarse_rows=8, decay=1.0)
    thetas = [lv["theta"] for lv in halved]
    assert thetas[0] == np.float32(0.08)
    for a, b in zip(thetas, thetas[1:]):
        assert b == np.float32(a * np.float32(0.5))
    assert all(lv["theta"] == np.float32(0.08) for lv in fixed)
    print("poisson3d(8): halved", [lv["n"] for lv in halved], "fixed", [lv["n"] for lv in fixed])
    assert [lv["n"] for lv in halved] != [lv["n"] for lv in fixed]


# ---- the exact cycle past the grid caps -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trip_levels(spmv):
    """name -> the two levels of a case of precond_trip_cases.SMOOTHED_CASES through the host twins, built once"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = pt.smoothed_hierarchy(spmv, pt.SMOOTHED_CASES[name][0])
        return built[name]
    return get


def test_the_fast_smoothed_prover_is_the_fraction_prover(spmv):
    n = pt.SMOOTHED_TWIN_ROWS
    levels = pt.smoothed_hierarchy(spmv, n)
    assert [lv["n"] for lv in levels] == [n, n // 2] and n // 2 > ac.DENSE_ROWS
    r = ac.exact_rhs(n)
    for pre, coarse, post in pt.SMOOTHED_TWIN_CHECKS:
        want, width = pt.prove_smoothed_vcycle_fractions(levels, r, pt.AMG_OMEGA, pre, post, coarse)
        got, got_width = pt.prove_smoothed_vcycle_fast(levels, r, pt.AMG_OMEGA, pre, post, coarse)
        assert want is not None and got is not None, (pre, coarse, post, width, got_width)
        assert got_width == width
        np.testing.assert_array_equal(bits(got), bits(want))
    # both refuse a right-hand side too wide for fp32, and the weight at which the coarse diagonal is 5/8
    wide = r * np.float32(1 << 20)
    assert pt.prove_smoothed_vcycle_fast(levels, wide, pt.AMG_OMEGA, 1, 1, 1)[0] is None
    assert pt.prove_smoothed_vcycle_fractions(levels, wide, pt.AMG_OMEGA, 1, 1, 1)[0] is None
    half = sc.hierarchy(spmv, *pt.tridiagonal(n), maps=ac.pair_maps(n, n // 2), weight=0.5)
    assert half[1]["va"][half[1]["ci"] == ac.rows_of(n // 2, half[1]["rp"])][5] == np.float32(0.625)
    assert pt.prove_smoothed_vcycle_fast(half, r, pt.AMG_OMEGA, 1, 1, 1)[0] is None
    assert pt.prove_smoothed_vcycle_fractions(half, r, pt.AMG_OMEGA, 1, 1, 1)[0] is None
    # the transfers alone: amg_smoothed_cases.prove_transfers' vectors and width on its three cases
    for name, level in transfer_levels(spmv):
        f, x, e = sc.exact_vectors(level)
        want_fc, want_x, width = sc.prove_transfers(level, f, x, e)
        res, fc, out, got_width = pt.prove_smoothed_transfers_fast(level, f, x, e)
        assert want_fc is not None and fc is not None and got_width == width, (name, width, got_width)
        np.testing.assert_array_equal(bits(fc), bits(want_fc), err_msg=name)
        np.testing.assert_array_equal(bits(out), bits(want_x), err_msg=name)
        np.testing.assert_array_equal(res.astype(np.float64), f - ac._spmv(level, x.astype(np.float64), np.float64))
    assert pt.prove_smoothed_transfers_fast(level, f * np.float32(1 << 22), x, e)[0] is None


@pytest.mark.parametrize("name", list(pt.SMOOTHED_CASES))
def test_every_smoothed_trip_case_is_admitted_and_passes_its_caps(trip_levels, name):
    n, lanes, sweep_counts = pt.SMOOTHED_CASES[name]
    levels = trip_levels(name)
    fine, coarse = levels
    count = n // 2
    assert n % 2 == 0 and [lv["n"] for lv in levels] == [n, count] == [fine["n"], fine["count"]]
    assert count > ac.DENSE_ROWS                                        # Jacobi-solved: no dense inverse
    # the caps: A and P have n rows, PT and level 1 have n / 2
    if name in ("L64", "L8"):
        assert pt.trips(n, row_trip(lanes)) == 3 and pt.trips(count, row_trip(lanes)) == 2
        assert pt.row_grid(count, 256 // lanes) == pt.ROW_BLOCKS and count - row_trip(lanes) == (5 if lanes == 64 else 33)
    elif name == "vec":
        assert count == pt.VEC_ROWS and pt.trips(n, VEC_TRIP) == 3 and pt.trips(count, VEC_TRIP) == 2
        # the library's own lane counts (pick_lanes_per_row, restated by exact_data.lanes_for): one lane for A, P and
        # PT, so the sweeps over A and P make a second trip of row_trip(1) rows; two lanes on level 1
        picked = [ed.lanes_for(m[1].size, rows) for m, rows in (((fine["rp"], fine["ci"]), n), (fine["P"], n),
                                                               (fine["PT"], count), ((coarse["rp"], coarse["ci"]), count))]
        assert picked == [1, 1, 1, 2] and pt.trips(n, row_trip(1)) == 2 and pt.trips(count, row_trip(2)) == 2
    else:
        assert lanes == 64 and count - row_trip(64) == {"below": -1, "at": 0, "above": 1}[name]
        assert pt.trips(n, row_trip(64)) == (2 if name == "below" else 3 if name == "above" else 2)
        assert n > row_trip(64) and pt.row_grid(count, 4) == pt.ROW_BLOCKS
        assert pt.trips(count, row_trip(64)) == (2 if name == "above" else 1)
    # what the issue worked out by hand, read from the host twins
    p_rp, p_ci, p_va = fine["P"]
    assert (p_va == np.float32(0.5)).all() and np.array_equal(np.diff(p_rp), np.r_[1, np.full(n - 2, 2), 1])
    rows = ac.rows_of(count, coarse["rp"])
    distance = np.abs(coarse["ci"] - rows)
    diagonal = coarse["va"][distance == 0]
    print(f"{name}: coarse diagonal in [{diagonal.min()}, {diagonal.max()}], {diagonal.size} rows")
    assert diagonal.size == count and (diagonal == np.float32(0.5)).all()
    assert (coarse["va"][distance == 1] == 0).all() and (coarse["va"][distance == 2] == np.float32(-0.25)).all()
    assert distance.max() == 2 and np.count_nonzero(distance == 1) == 2 * (count - 1)
    assert np.array_equal(ac.diag32(count, coarse["rp"], coarse["ci"], coarse["va"]), np.full(count, 0.5, np.float32))
    # the transfer test's vectors: integers in [-8, 8] for f, x and e
    f, x, e = sc.exact_vectors(fine)
    res, fc, out, width = pt.prove_smoothed_transfers_fast(fine, f, x, e)
    print(f"{name}: the transfers on integer f, x, e: " + (f"{width} bits" if res is not None else f"not admitted ({width})"))
    assert res is not None and width < 24, (name, width)
    np.testing.assert_array_equal(res.astype(np.float64), f - ac._spmv(fine, x.astype(np.float64), np.float64))
    np.testing.assert_array_equal(fc.astype(np.float64), sc._matvec(count, fine["PT"], res.astype(np.float64), np.float64))
    np.testing.assert_array_equal(out.astype(np.float64), x + sc._matvec(n, fine["P"], e.astype(np.float64), np.float64))
    r = ac.exact_rhs(n)
    for pre, coarse_sweeps, post in sweep_counts:
        z, width = pt.prove_smoothed_vcycle_fast(levels, r, pt.AMG_OMEGA, pre, post, coarse_sweeps)
        print(f"{name}: n = {n}, (pre, coarse, post) = {(pre, coarse_sweeps, post)}: " +
              (f"{width} bits" if z is not None else f"not admitted ({width})"))
        assert z is not None, (name, pre, coarse_sweeps, post, width)
        assert width < 24 and np.abs(z).max() > 0
        # everything is exact, so any order of evaluation gives the same floats: both numpy cycles
        for dtype in (np.float32, np.float64):
            other = sc.vcycle(levels, r, pt.AMG_OMEGA, pre, post, coarse_sweeps, dtype)
            np.testing.assert_array_equal(bits(other.astype(np.float32)), bits(z), err_msg=f"{name} {dtype.__name__}")
            np.testing.assert_array_equal(other.astype(np.float64), z.astype(np.float64))


# ---- rejections without a device -------------------------------------------------------------------------------
def test_prolongator_checks_in_the_stated_order_with_nothing_written(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    f32 = lambda v: np.asarray(v, np.float32)
    A = spmv.csr_from_arrays(3, 3, [0, 2, 3, 5], [0, 1, 1, 1, 2], f32([2, -1, 2, -1, 2]))
    R = spmv.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], f32([1, 1]))
    P = spmv.csr_from_arrays(1, 1, [0, 1], [0], f32([7]))
    agg = np.array([0, 0, 1], np.int32)
    ptr = agg.ctypes.data_as(ctypes.c_void_p)
    untouched = lambda: (P.contents.num_rows, P.contents.nnz, float(P.contents.values[0])) == (1, 1, 7.0)
    assert lib.spmv_c_amg_prolongator_cpu_csr(None, A, ptr, 2, 0.5) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, None, ptr, 2, 0.5) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, A, None, 2, 0.5) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, R, ptr, 2, -1.0) == E.INVALID_DIMENSION
    for rp, ci in (([0, 2, 3, 4], [0, 1, 1, 1, 2]), ([1, 2, 3, 5], [0, 1, 1, 1, 2]), ([0, 3, 2, 5], [0, 1, 1, 1, 2]),
                   ([0, 2, 3, 5], [0, 1, 1, 3, 2]), ([0, 2, 3, 5], [0, -1, 1, 1, 2])):
        X = spmv.csr_from_arrays(3, 3, rp, ci, f32([2, -1, 2, -1, 2]))
        assert lib.spmv_c_amg_prolongator_cpu_csr(P, X, ptr, 2, -1.0) == E.INVALID_FORMAT, (rp, ci)
        spmv.csr_destroy(X)
    D = spmv.csr_wrap_device(3, 3, 5, FAKE_RP, FAKE_CI, FAKE_VA)                 # no host arrays
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, D, ptr, 2, 0.5) == E.INVALID_FORMAT
    for weight in (0.0, 2.0, -0.5, float("nan")):
        assert lib.spmv_c_amg_prolongator_cpu_csr(P, A, ptr, 2, weight) == E.INVALID_ARGUMENT, weight
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, A, ptr, 0, 0.5) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, A, ptr, 1, 0.5) == E.INVALID_ARGUMENT          # entry 1 out of range
    for bad in (np.array([0, -1, 1], np.int32), np.array([0, 2, 1], np.int32)):
        assert spmv.amg_prolongator_cpu_csr(P, A, bad, 2, 0.5) == E.INVALID_ARGUMENT
    for value in (0.0, -2.0, float("inf")):                                      # a bad diagonal in row 1
        X = spmv.csr_from_arrays(3, 3, [0, 2, 3, 5], [0, 1, 1, 1, 2], f32([2, -1, value, -1, 2]))
        assert lib.spmv_c_amg_prolongator_cpu_csr(P, X, ptr, 2, 0.5) == E.INVALID_ARGUMENT, value
        spmv.csr_destroy(X)
    N = spmv.csr_from_arrays(3, 3, [0, 2, 2, 4], [0, 1, 1, 2], f32([2, -1, -1, 2]))   # row 1 stores no diagonal
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, N, ptr, 2, 0.5) == E.INVALID_ARGUMENT
    assert untouched()
    assert lib.spmv_c_amg_prolongator_cpu_csr(P, A, ptr, 2, 0.5) == 0 and P.contents.num_rows == 3
    for M in (A, R, P, D, N):
        spmv.csr_destroy(M)


def test_setup_and_transfer_checks_before_any_device_work(spmv):
    E = spmv.SpMVError
    A = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    R = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], np.ones(2, np.float32))    # host only
    lib = spmv.lib()
    bad_cfg, bad_sm = spmv.AMGConfig(max_levels=0), spmv.AMGSmoothing(prolongator_weight=2.0)
    bad_map = [np.array([0, 0, 1, 1, 2, 2, 3, 8], np.int32)]
    for setup in (lambda M, c, s, m: spmv.amg_setup_smoothed(M, c, s, m),
                  lambda M, c, s, m: spmv.amg_setup_smoothed_device(M, c, s)):
        out = spmv.AMGResult(error_code=7, levels=9)
        # amg_setup's order: the matrix, then the config, then the smoothing, then the aggregates
        for M, cfg, sm, code in ((None, bad_cfg, bad_sm, E.INVALID_ARGUMENT), (R, bad_cfg, bad_sm, E.INVALID_DIMENSION),
                                 (H, bad_cfg, bad_sm, E.INVALID_FORMAT), (A, bad_cfg, bad_sm, E.INVALID_ARGUMENT)):
            res, handle = setup(M, cfg, sm, bad_map)
            assert res.error_code == code and handle is None and (res.levels, res.bad_row, res.bad_level) == (0, -1, -1)
        for field, value in (("prolongator_weight", 0.0), ("prolongator_weight", 2.0), ("prolongator_weight", -1.0),
                             ("prolongator_weight", float("nan")), ("strength_decay", 0.0), ("strength_decay", 1.5),
                             ("strength_decay", -0.5), ("strength_decay", float("nan"))):
            res, handle = setup(A, None, spmv.AMGSmoothing(**{field: value}), bad_map)
            assert res.error_code == E.INVALID_ARGUMENT and handle is None, (field, value)
    res, handle = spmv.amg_setup_smoothed(A, None, None, bad_map)
    assert res.error_code == E.INVALID_ARGUMENT and handle is None
    handle = ctypes.c_void_p(0x1234)
    assert lib.spmv_c_amg_setup_smoothed(ctypes.byref(handle), None, None, None, 0, None, None) == E.INVALID_ARGUMENT
    assert handle.value is None                                                  # *out is null on failure
    handle = ctypes.c_void_p(0x1234)
    assert lib.spmv_c_amg_setup_smoothed_device(ctypes.byref(handle), None, None, None, 0, None) == E.INVALID_ARGUMENT
    assert handle.value is None
    assert lib.spmv_c_amg_setup_smoothed(None, A, None, None, 0, None, None) == E.INVALID_ARGUMENT
    # null hierarchies
    assert spmv.amg_is_smoothed(None) == 0
    assert spmv.amg_level_transfer(None, 0)[0] == E.INVALID_ARGUMENT
    assert spmv.amg_restrict(None, 0, 0x1000, 0x2000, 0x3000) == E.INVALID_ARGUMENT
    assert spmv.amg_prolong(None, 0, 0x1000, 0x2000) == E.INVALID_ARGUMENT
    for M in (A, R, H):
        spmv.csr_destroy(M)


# ---- the sanitized caller --------------------------------------------------------------------------------------
def test_amg_smoothed_host_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-amg-smoothed builds tests/cpp/bin/amg_smoothed_host_sanitized (csrc/amg_host.cpp,
    the host twins it calls and tests/cpp/amg_smoothed_host_sanitized.cpp under AddressSanitizer + UBSan); any
    sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-amg-smoothed"],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "amg_smoothed_host_sanitized")],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
