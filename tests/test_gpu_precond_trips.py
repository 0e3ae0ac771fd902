"""The preconditioner kernels past their grid caps: ic0_csr, ilu0_csr, sptrsv_csr_multi, fsai_csr, the AMG V-cycle and
the device-side AMG setup, every comparison at zero tolerance (bits of values, a NaN by position where the module the
helper comes from compares so; ints of structure).

csrc/device_common.h caps a row kernel's grid at 2048 workgroups of 256 threads (R_L = 524 288 / L rows a trip at L
lanes per row) and an element-wise kernel's at 1024 (V = 262 144 elements a trip).  The shapes of
tests/precond_trip_cases.py are just larger, so each grid-stride loop below goes round a second time (a third on the
fine AMG level), and tests/test_precond_trips_host.py proves on the CPU that they are and that the expected values are
exact.  SPMV_DEBUG forces the lane counts; every test that sets it removes it in a `finally` (forced()).

kernel                                   case that gives it a second trip                     rows in that trip
factor0_kernel<IC0 | ILU0, 64>           exact and random 3 x 3 pieces, 8197 a level          5 of each of 3 levels
factor0_kernel<IC0 | ILU0, 8>            the same, 65 569 a level                             33 of each of 3 levels
factor0_pivot_kernel<IC0 | ILU0>         diag(4) of V + 257 rows, bad rows >= V               257
sptrsv_multi_kernel<64, 4, 8, false>     two_level_triangle(64), k = 9 (windows 0-3, 4-7, 8)  5 of each of 2 levels
sptrsv_multi_kernel<8, 8, 8, false>      two_level_triangle(8), k = 9 (windows 0-7, 8)        33 of each of 2 levels
sptrsv_multi_kernel<1, 8, 8, true>       two_level_triangle(1), k = 5, ordered = 1            257 of each of 2 levels
  (each switched band below once more with 64 further rows, "deep": precond_trip_cases' docstring)
fsai_numeric_kernel<4, 64>, <8, 64>      switched band, n = 8197 (4 rows a workgroup)         5
fsai_numeric_kernel<8, 64>               342 proved periods of 24 rows, n = 8208              16
fsai_numeric_kernel<16, 8>               switched band, n = 65 569 (32 rows a workgroup)      33
fsai_numeric_kernel<32, 16>              switched band, n = 16 393 (8 rows a workgroup)       9
fsai_numeric_kernel<64, 1>, <64, 64>     switched band, n = 6148 (3 rows a workgroup)         4
fsai_count_kernel, fsai_columns_kernel,  tridiag(-1, 2, -1) of V + 257 rows, each defect in   258 (count: rows and the
fsai_bad_row_kernel                      a row >= V                                           end slot), 257
amg_sweep_kernel<64>                     tridiagonal(16 394): fine level, coarse level        8192 + 10, 5
amg_restrict_kernel<64>                  the same: 8197 aggregates                            5
amg_sweep_kernel<8>, amg_restrict_<8>    tridiagonal(131 138)                                 65 536 + 66, 33; 33
amg_scale_kernel, amg_correct_kernel     tridiagonal(2 (V + 257)), the library's lanes        V + 514 (fine), 257 (scale, coarse)
mis2_round_kernel<64>, mis2_phase1_<64>, poisson2d(96): 2304 workgroups asked for, 2048 run:  1024
mis2_phase2_kernel<64>, min_fold_kernel  Scratch::partial is full
mis2_round_<8>, phase1_<8>, phase2_<8>   poisson2d(257)                                       513
mis2_init_kernel, mis2_flags_kernel,     tridiag(-1, 2, -1) of V + 257 rows                   257 (258 where the loop
the device scan, amg_prolongation_kernel                                                      takes the end slot)
amg_diag_kernel, min_fold_kernel         the same with a zero diagonal in a row >= V          257; 1024 partials

The FSAI exact tier repeats one period proved by fsai_cases.prove_exact (precond_trip_cases' docstring says why).
The smoothed-aggregation AMG (amg_residual_kernel, amg_restrict_weighted_kernel, amg_prolong_kernel,
amg_smoothing_scale_kernel and the refill of amg_update) has the same pass in tests/test_gpu_amg_smoothed_trips.py,
which lists its kernels and caps."""
import contextlib
import functools
import importlib
import os

import numpy as np
import pytest

import amg_cases as ac
import exact_data as ed
import fsai_cases as fc
import precond_trip_cases as pt
from test_fsai_host import bits, host_fsai

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
sptrsv_tests = importlib.import_module("test_gpu_sptrsv")
multi_tests = importlib.import_module("test_gpu_sptrsv_multi")
ic0_tests = importlib.import_module("test_gpu_ic0")
ilu0_tests = importlib.import_module("test_gpu_ilu0")
fsai_tests = importlib.import_module("test_gpu_fsai")
amg_tests = importlib.import_module("test_gpu_amg")
setup_tests = importlib.import_module("test_gpu_amg_setup_device")

FACTOR = {"ic": (ic0_tests._factor, "ic0_cpu_csr", "ic0_lanes", "bad_pivot"),
          "ilu": (ilu0_tests._factor, "ilu0_cpu_csr", "ilu0_lanes", "zero_pivot")}


@contextlib.contextmanager
def forced(value):
    """SPMV_DEBUG = value inside the block (None: unset), removed afterwards whatever happens"""
    os.environ.pop("SPMV_DEBUG", None)
    if value is not None:
        os.environ["SPMV_DEBUG"] = value
    try:
        yield
    finally:
        os.environ.pop("SPMV_DEBUG", None)


def assert_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(what))


# ------------------------------------------------------------------------------------------ 1. IC(0) and ILU(0)
@pytest.mark.parametrize("L", pt.TRIP_LANES)
@pytest.mark.parametrize("kind", pt.FACTOR_KINDS)
def test_factor_three_wide_levels_past_the_grid_cap(gpu, kind, L):
    """factor0_kernel<KIND, L> on three levels of R_L + 256 / L + 1 rows each: the exact tier against the proved
    factor and the CPU's, the random tier against the CPU's; out of place and in place."""
    factor, cpu_name, key, pivot_field = FACTOR[kind]
    blocks = pt.factor_blocks(L)
    n, rp, ci, va, fact = pt.exact_factor_blocks(kind, blocks)
    proved, _ = pt.prove_chain_exact(kind, n, rp, ci, va)
    assert_bits(proved, fact, "the construction's factor")
    for tier, matrix, expected in (("exact", (n, rp, ci, va), proved), ("random", pt.random_factor_blocks(kind, blocks), None)):
        A = sptrsv_tests._upload(gpu, *matrix)
        try:
            cpu, cpu_pivot = getattr(gpu, cpu_name)(A)
            assert cpu_pivot == -1
            if expected is not None:
                assert_bits(cpu, expected, "the CPU's factor")
            with forced(f"{key}={L}"):
                for in_place in (False, True):
                    res, got = factor(gpu, A, matrix[3], in_place)
                    what = (kind, tier, L, in_place, res.num_levels, res.launches, res.lanes_per_row)
                    assert res.error_code == 0 and getattr(res, pivot_field) == -1, what
                    assert (res.launches, res.num_levels, res.lanes_per_row) == (3, 3, L), what
                    assert_bits(got, cpu, what)
                    if expected is not None:
                        assert_bits(got, expected, what)
        finally:
            gpu.csr_destroy(A)


@pytest.mark.parametrize("kind", pt.FACTOR_KINDS)
def test_pivot_scan_second_trip(gpu, kind):
    """factor0_pivot_kernel<KIND> over V + 257 rows whose bad diagonals (negative, NaN, zero, in that order) lie in
    rows >= V: the lowest bad row under each rule, and -1 on the clean copy."""
    factor, cpu_name, _, pivot_field = FACTOR[kind]
    for clean in (False, True):
        n, rp, ci, va = pt.pivot_scan_matrix(clean)
        A = sptrsv_tests._upload(gpu, n, rp, ci, va)
        try:
            cpu, cpu_pivot = getattr(gpu, cpu_name)(A)
            assert cpu_pivot == (-1 if clean else pt.PIVOT_BAD[kind])
            for in_place in (False, True):
                res, got = factor(gpu, A, va, in_place)
                what = (kind, clean, in_place, getattr(res, pivot_field))
                assert res.error_code == 0 and getattr(res, pivot_field) == cpu_pivot, what
                np.testing.assert_array_equal(np.isnan(got), np.isnan(cpu), err_msg=str(what))
                keep = ~np.isnan(cpu)
                assert_bits(got[keep], cpu[keep], what)
        finally:
            gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------------ 2. sptrsv_csr_multi
@pytest.mark.parametrize("L,uplo,unit", pt.MULTI_CASES)
def test_multi_solve_two_wide_levels_past_the_grid_cap(gpu, L, uplo, unit):
    """sptrsv_multi_kernel<L, W, 8, false> with k = 9 on two levels of R_L + 256 / L + 1 rows: X is the integer
    matrix bit for bit, column j is sptrsv_csr on that column, out of place and in place."""
    case = ed.two_level_triangle(L, uplo, unit)
    X, B, _ = pt.multi_rhs(case, pt.MULTI_K)
    dev = multi_tests.Device(gpu, case["n"], case["rp"], case["ci"], case["va"])
    try:
        with forced(f"sptrsv_lanes={L}"):
            cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit)
            ref, singles = dev.singles(B, cfg)
            assert (ref.num_levels, ref.launches, ref.lanes_per_row) == (2, 2, L)
            assert_bits(singles, X, ("sptrsv_csr per column", L, uplo, unit))
            for in_place in (False, True):
                res, got = dev.multi(B, cfg, in_place=in_place)           # poisoned X, guarded views
                what = (L, uplo, unit, in_place, res.num_levels, res.launches, res.lanes_per_row)
                assert res.error_code == 0 and (res.num_levels, res.launches, res.lanes_per_row) == (2, 2, L), what
                assert_bits(got, X, what)
                assert_bits(got, singles, what)
    finally:
        dev.close()


@pytest.mark.parametrize("uplo,unit", pt.ORDERED_CASES)
def test_ordered_multi_solve_past_the_one_lane_cap(gpu, uplo, unit):
    """ordered = 1 is one lane per row whatever sptrsv_lanes says, so its cap is R_1: two_level_triangle(1, ...) with
    k = 5 under sptrsv_lanes=8, against sptrsv_cpu_csr column by column and the integers."""
    case = ed.two_level_triangle(1, uplo, unit)
    X, B, _ = pt.multi_rhs(case, pt.ORDERED_K)
    dev = multi_tests.Device(gpu, case["n"], case["rp"], case["ci"], case["va"])
    try:
        with forced("sptrsv_lanes=8"):
            cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit, ordered=1)
            cpu = np.stack([gpu.sptrsv_cpu_csr(dev.A, B[:, j], cfg) for j in range(pt.ORDERED_K)], axis=1)
            assert_bits(cpu, X, "sptrsv_cpu_csr per column")
            for in_place in (False, True):
                res, got = dev.multi(B, cfg, in_place=in_place)
                what = (uplo, unit, in_place, res.num_levels, res.launches)
                assert res.error_code == 0 and (res.num_levels, res.launches) == (2, 2), what
                assert_bits(got, cpu, what)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. FSAI
@pytest.mark.parametrize("cls,L,order", pt.FSAI_TRIP_CASES)
def test_fsai_numeric_kernel_second_trip(gpu, cls, L, order):
    """fsai_numeric_kernel<cls, L> on 2048 G + G + 1 (+ 64) rows whose length changes at row 2048 G: G is fsai_cpu_csr's in
    row pointers, columns and value bits; the refill after a value change equals a fresh build and the CPU's."""
    n, rp, ci, va = pt.fsai_trip_matrix(cls, L, order)
    new_va = pt.rescaled(n, rp, ci, va)
    (status, bad, want), (status2, bad2, want2) = host_fsai(gpu, n, rp, ci, va), host_fsai(gpu, n, rp, ci, new_va)
    assert (status, bad, status2, bad2) == (0, -1, 0, -1)
    A, A2 = fsai_tests._upload(gpu, n, rp, ci, va), fsai_tests._upload(gpu, n, rp, ci, new_va)
    G, fresh = gpu.csr_create(1, 1, 0), gpu.csr_create(1, 1, 0)
    tag = f"class {cls} lanes {L} {order}"
    try:
        with forced(f"fsai_lanes={L},fsai_class={cls}"):
            res = gpu.fsai_csr(G, A)
            assert (res.error_code, res.bad_row, res.long_row) == (0, -1, -1), tag
            assert (res.nnz, res.max_row, res.row_class, res.lanes_per_row) == (want[1].size, cls, cls, L), tag
            fsai_tests._check_equal(fsai_tests._read(gpu, G), want, tag)
            res = gpu.fsai_csr_numeric(G, A2)
            assert (res.error_code, res.bad_row, res.row_class, res.lanes_per_row) == (0, -1, cls, L), tag
            refilled = fsai_tests._read(gpu, G)
            fsai_tests._check_equal(refilled, want2, tag + " refill")
            assert gpu.fsai_csr(fresh, A2).error_code == 0
            fsai_tests._check_equal(refilled, fsai_tests._read(gpu, fresh), tag + " refill against a fresh build")
    finally:
        for M in (A, A2, G, fresh):
            gpu.csr_destroy(M)


def test_fsai_exact_tier_past_the_grid_cap(gpu):
    """342 proved periods of 24 rows at fsai_lanes=64: class 8, 4 rows a workgroup, 8208 rows > 8192."""
    n, rp, ci, va = pt.fsai_exact_matrix()
    want = pt.fsai_exact_expected()
    n0, _, _, _, L0 = pt.fsai_exact_period()
    A = fsai_tests._upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    try:
        with forced(f"fsai_lanes={pt.FSAI_EXACT_LANES}"):
            res = gpu.fsai_csr(G, A)
        assert (res.error_code, res.bad_row, res.max_row, res.row_class) == (0, -1, 6, 8)
        assert res.lanes_per_row == pt.FSAI_EXACT_LANES
        g_rp, g_ci, g = fsai_tests._read(gpu, G)
        fsai_tests._check_equal((g_rp, g_ci, g), want, "the proved period, repeated")
        # G L = I, period by period (G is block diagonal: every column of a row lies in the row's period)
        rows = fc.rows_of(n, g_rp)
        assert np.array_equal(rows // n0, g_ci // n0)
        dense = np.zeros((pt.FSAI_PERIODS, n0, n0))
        dense[rows // n0, rows % n0, g_ci % n0] = g
        assert np.array_equal(dense @ L0.astype(np.float64), np.broadcast_to(np.eye(n0), dense.shape))
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(G)


@functools.lru_cache(maxsize=None)
def structure_reference():
    spmv = importlib.import_module("gpu-spmv_amd")
    status, bad, want = host_fsai(spmv, *pt.fsai_structure_matrix())
    assert (status, bad) == (0, -1)
    for a in want:
        a.setflags(write=False)
    return want


def test_fsai_structure_kernels_second_trip(gpu):
    """fsai_count_kernel, fsai_columns_kernel and fsai_bad_row_kernel over V + 257 rows: the clean build is the
    CPU's; each rejected variant, its defect in a row >= V, gives the CPU's code and leaves G as it was; a negative
    diagonal in a row >= V is reported as the CPU reports it."""
    want = structure_reference()
    n, rp, ci, va = pt.fsai_structure_matrix()
    A = fsai_tests._upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    try:
        res = gpu.fsai_csr(G, A)
        assert (res.error_code, res.bad_row, res.long_row, res.max_row) == (0, -1, -1, 2)
        fsai_tests._check_equal(fsai_tests._read(gpu, G), want, "clean")
        for defect in ("unsorted", "no_diagonal", "wild_column", "long_row"):
            m = pt.fsai_structure_matrix(defect)
            code = host_fsai(gpu, *m)[0]
            assert code != 0, defect
            B = fsai_tests._upload(gpu, *m)
            res = gpu.fsai_csr(G, B)
            gpu.csr_destroy(B)
            assert res.error_code == code, (defect, res.error_code, code)
            if defect == "long_row":
                assert (res.long_row, res.max_row) == (pt.FSAI_DEFECT_ROWS[defect], fc.MAX_ROW + 1)
            fsai_tests._untouched(gpu, G, want)
        m = pt.fsai_structure_matrix("bad_row")
        status, cpu_bad, cpu = host_fsai(gpu, *m)
        assert status == 0 and cpu_bad == pt.FSAI_DEFECT_ROWS["bad_row"]
        B = fsai_tests._upload(gpu, *m)
        res = gpu.fsai_csr(G, B)
        assert (res.error_code, res.bad_row) == (0, cpu_bad)
        got = fsai_tests._read(gpu, G)
        assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1])
        assert np.array_equal(np.isnan(got[2]), np.isnan(cpu[2])) and np.isnan(cpu[2]).any()
        keep = ~np.isnan(cpu[2])
        assert_bits(got[2][keep], cpu[2][keep], "bad_row")
        assert gpu.fsai_csr_numeric(G, B).bad_row == cpu_bad
        gpu.csr_destroy(B)
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(G)


# ------------------------------------------------------------------------------------------ 4. AMG V-cycle
def apply_through_views(gpu, h, r):
    """amg_apply on views 3 floats into larger buffers (test_gpu_amg's layout): z, with the guards asserted intact"""
    n, front, back = h.n, 3, 5
    d_in, d_out = gpu.CudaBuffer(front + n + back), gpu.CudaBuffer(front + n + back)
    try:
        padded = np.full(front + n + back, np.nan, np.float32)    # NaN padding: a read of it would poison the result
        padded[front:front + n] = r
        d_in.copyFromHost(padded, padded.size)
        marks = np.arange(front + n + back, dtype=np.float32) + 0.5
        d_out.copyFromHost(marks, marks.size)
        assert gpu.amg_apply(h.H, d_in.get() + 4 * front, d_out.get() + 4 * front) == 0
        got = d_out.copyToHost(marks.size)
        assert_bits(got[:front], marks[:front], "front guard")
        assert_bits(got[front + n:], marks[front + n:], "back guard")
        assert_bits(d_in.copyToHost(padded.size), padded, "the input")
        return got[front:front + n]
    finally:
        d_in.release()
        d_out.release()


@pytest.mark.parametrize("name", list(pt.AMG_CASES))
def test_vcycle_every_kernel_past_its_cap(gpu, name):
    """tridiag(-1, 2, -1) with pair aggregates, two levels, the coarsest Jacobi-solved, omega = 1/2: z is the proved
    bits (precond_trip_cases.prove_vcycle_fast decides; nothing is measured here), twice, and through views."""
    n, lanes, sweep_counts = pt.AMG_CASES[name]
    matrix, r, maps = pt.tridiagonal(n), ac.exact_rhs(n), ac.pair_maps(n, n // 2)
    for pre, coarse, post in sweep_counts:
        want, width = pt.prove_vcycle_fast(n, n // 2, r, pt.AMG_OMEGA, pre, post, coarse)
        assert want is not None, (name, pre, coarse, post, width)
        cfg = gpu.AMGConfig(jacobi_weight=pt.AMG_OMEGA, pre_sweeps=pre, post_sweeps=post, coarse_sweeps=coarse)
        h = amg_tests.Hier(gpu, *matrix, cfg=cfg, maps=maps)
        try:
            assert (h.res.error_code, h.res.levels, h.res.coarse_solver) == (0, 2, 1), (name, h.res.error_code)
            with forced(None if lanes is None else f"amg_lanes={lanes}"):
                what = (name, pre, coarse, post)
                assert_bits(h.apply(r), want, what)
                assert_bits(h.apply(r), want, what + ("again",))
                assert_bits(apply_through_views(gpu, h, r), want, what + ("views",))
        finally:
            h.close()


# ------------------------------------------------------------------------------------------ 5. AMG setup on the device
@pytest.mark.parametrize("grid,lanes", [(pt.MIS_CAP_GRID, 64), (pt.MIS_L8_GRID, 8)])
def test_mis2_aggregation_at_and_past_the_grid_cap(gpu, grid, lanes):
    """mis2_round_kernel, mis2_phase1_kernel and mis2_phase2_kernel<lanes> with 2048 workgroups, one partial each for
    min_fold_kernel (Scratch::partial holds exactly that many), and a second trip: amg_aggregate_mis2_cpu_csr's ints."""
    level = setup_tests.Level(gpu, *spd.poisson2d(grid))
    try:
        with forced(f"mis_lanes={lanes}"):
            for seed in pt.MIS_SEEDS:
                level.check(0.08, seed, what=(grid, lanes, seed))
    finally:
        level.close()


def test_mis2_element_wise_kernels_second_trip(gpu):
    """mis2_init_kernel, mis2_flags_kernel, the device scan and the phases over V + 257 rows at the library's lanes"""
    level = setup_tests.Level(gpu, *pt.tridiagonal(pt.VEC_ROWS))
    try:
        with forced(None):
            for seed in pt.MIS_SEEDS:
                level.check(0.08, seed, what=("path", seed))
    finally:
        level.close()


def test_device_setup_past_the_vector_cap(gpu):
    """amg_setup_device on tridiag(-1, 2, -1) of V + 257 rows, max_levels = 2: level 1 is amg_setup's, handed the
    definition's map, bit for bit (amg_prolongation_kernel, amg_diag_kernel and the products past V); a zero diagonal
    in a row >= V is reported with its row and level 0 (amg_diag_kernel's second trip, min_fold_kernel over 1024
    partials), and so is one in the last workgroup's first trip (the last partial)."""
    n, rp, ci, va = pt.tridiagonal(pt.VEC_ROWS)
    cfg = gpu.AMGConfig(max_levels=2)
    host_A = gpu.csr_from_arrays(n, n, rp, ci, va)
    status, agg, count, rounds = gpu.amg_aggregate_mis2_cpu_csr(host_A, cfg.strength, 0)
    gpu.csr_destroy(host_A)
    assert status == 0 and ac.DENSE_ROWS < count < n
    dev = setup_tests.DeviceHier(gpu, n, rp, ci, va, cfg, 0)
    host = amg_tests.Hier(gpu, n, rp, ci, va, cfg, [agg])
    try:
        assert dev.res.error_code == 0 and dev.H is not None and (dev.res.bad_row, dev.res.bad_level) == (-1, -1)
        assert host.res.error_code == 0
        assert (dev.res.levels, dev.res.coarse_solver) == (host.res.levels, host.res.coarse_solver) == (2, 1)
        got, want = dev.levels(), host.levels()
        assert got[1]["n"] == count
        amg_tests.assert_levels_equal(got, want, "the device-built hierarchy")
        assert 1 <= gpu.amg_setup_rounds(dev.H, 0) <= rounds
        r = ac.exact_rhs(n)
        assert_bits(dev.apply(r), host.apply(r), "one V-cycle of each hierarchy")
    finally:
        dev.close()
        host.close()
    diagonal = np.flatnonzero(ci == ac.rows_of(n, rp))
    for row in (pt.SETUP_BAD_ROW, pt.SETUP_LAST_PARTIAL_ROW):            # the second trip; the last slot min_fold reads
        bad = va.copy()
        bad[diagonal[row]] = 0.0
        h = setup_tests.DeviceHier(gpu, n, rp, ci, bad, cfg, 0)
        try:
            assert h.H is None
            assert (h.res.error_code, h.res.bad_level, h.res.bad_row) == (gpu.SpMVError.INVALID_ARGUMENT, 0, row)
        finally:
            h.close()
