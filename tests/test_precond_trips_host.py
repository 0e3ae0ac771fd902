"""The claims of tests/precond_trip_cases.py, proved on the CPU (no GPU): that every shape passes the grid cap it is
there for, computed from exact_data's constants, and that every "exact" there is exact: the vectorised provers
against the Python-loop provers of ic0_cases, ilu0_cases, fsai_cases and amg_cases on small copies of the same
constructions, and then on the full shapes."""
import importlib

import numpy as np
import pytest

import amg_cases as ac
import exact_data as ed
import fsai_cases as fc
import ic0_cases
import ilu0_cases
import precond_trip_cases as pt
from exact_data import EXACT_LIMIT, VEC_TRIP, row_trip
from test_fsai_host import bits, host_fsai

spd = importlib.import_module("gpu-spmv_amd.spd")

LOOP_PROVERS = {"ic": ic0_cases.prove_exact, "ilu": ilu0_cases.prove_exact}


def cpu_factor(spmv, kind, n, rp, ci, va):
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    try:
        return (spmv.ic0_cpu_csr if kind == "ic" else spmv.ilu0_cpu_csr)(A)
    finally:
        spmv.csr_destroy(A)


def test_the_constants_are_the_launch_layers():
    assert (pt.BLOCK, pt.ROW_BLOCKS, pt.VEC_BLOCKS) == (256, 2048, 1024)
    assert pt.VEC_ROWS == ed.TILED_TRIP_SIZE and pt.trips(pt.VEC_ROWS, VEC_TRIP) == 2
    assert pt.vec_grid(pt.VEC_ROWS) == pt.VEC_BLOCKS and pt.VEC_ROWS - VEC_TRIP == pt.BLOCK + 1
    for L in pt.TRIP_LANES:
        n = pt.past_row_cap(L)
        assert n == ed.LANE_SIZES[L] and pt.row_grid(n, pt.BLOCK // L) == pt.ROW_BLOCKS
        assert pt.trips(n, row_trip(L)) == 2 and n - row_trip(L) == pt.BLOCK // L + 1
    # Slab<CLASS> and groups_per_wave<CLASS, LANES> of csrc/fsai.hip, restated
    for cls in fc.CLASSES:
        slab = cls * (cls + 1) // 2 * 8 + cls * 8 + cls * 4
        assert pt.FSAI_FIT[cls] == max(12288 // slab, 1) and pt.FSAI_WAVES[cls] == (3 if cls == 64 else 4)
        assert pt.FSAI_WAVES[cls] * pt.FSAI_FIT[cls] * slab <= 65536
    assert [pt.FSAI_ROWS_PER_BLOCK(c, L) for c, L in pt.FSAI_TRIP_PAIRS] == [4, 4, 32, 8, 3, 3]
    assert {c for c, _ in pt.FSAI_TRIP_PAIRS} == set(fc.CLASSES)
    n, rp, ci, va = ac.tridiagonal(37)
    for got, want in zip(pt.tridiagonal(37), (n, rp, ci, va)):
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------ 1. IC(0) and ILU(0)
@pytest.mark.parametrize("kind", pt.FACTOR_KINDS)
def test_the_chain_prover_is_the_loop_prover_on_a_small_copy(spmv, kind):
    n, rp, ci, va, fact = pt.exact_factor_blocks(kind, pt.PROOF_BLOCKS)
    proved, level = pt.prove_chain_exact(kind, n, rp, ci, va)
    np.testing.assert_array_equal(bits(proved), bits(LOOP_PROVERS[kind](n, rp, ci, va)))
    np.testing.assert_array_equal(bits(proved), bits(fact))
    got, pivot = cpu_factor(spmv, kind, n, rp, ci, va)
    assert pivot == -1
    np.testing.assert_array_equal(bits(got), bits(fact))
    assert np.bincount(level).tolist() == [pt.PROOF_BLOCKS] * 3
    # the prover refuses what is not exact: one value off by one
    wrong = va.copy()
    wrong[rp[int(np.flatnonzero(level == 2)[0])]] += 1.0
    with pytest.raises(AssertionError):
        pt.prove_chain_exact(kind, n, rp, ci, wrong)


@pytest.mark.parametrize("L", pt.TRIP_LANES)
@pytest.mark.parametrize("kind", pt.FACTOR_KINDS)
def test_three_levels_each_past_the_row_cap(spmv, kind, L):
    blocks = pt.factor_blocks(L)
    assert pt.trips(blocks, row_trip(L)) == 2 and blocks - row_trip(L) == 256 // L + 1
    assert pt.row_grid(blocks, 256 // L) == pt.ROW_BLOCKS
    n, rp, ci, va, fact = pt.exact_factor_blocks(kind, blocks)
    proved, level = pt.prove_chain_exact(kind, n, rp, ci, va)
    np.testing.assert_array_equal(bits(proved), bits(fact))
    got, pivot = cpu_factor(spmv, kind, n, rp, ci, va)
    assert pivot == -1
    np.testing.assert_array_equal(bits(got), bits(fact))
    for matrix in ((n, rp, ci), pt.random_factor_blocks(kind, blocks)[:3]):
        status, level_ptr, order, levels, missing = spmv.sptrsv_levels(*matrix, 0)
        assert (status, levels, missing) == (0, 3, -1)
        assert np.diff(level_ptr).tolist() == [blocks] * 3
        assert not np.array_equal(order, np.arange(n))                       # level order is not row order
        assert not np.array_equal(np.sort(order[:blocks]), 3 * np.arange(blocks))      # nor is row 3 b + j the layout
    np.testing.assert_array_equal(np.sort(order[:blocks]), np.flatnonzero(level == 0))
    # the inexact tier factors cleanly on the CPU
    m = pt.random_factor_blocks(kind, blocks)
    got, pivot = cpu_factor(spmv, kind, *m)
    assert pivot == -1 and np.isfinite(got).all()
    assert not np.array_equal(got, np.rint(got))


@pytest.mark.parametrize("kind", pt.FACTOR_KINDS)
def test_the_pivot_scan_meets_its_bad_rows_in_the_second_trip_only(spmv, kind):
    n, rp, ci, va = pt.pivot_scan_matrix()
    assert n == pt.VEC_ROWS and pt.trips(n, VEC_TRIP) == 2 and min(pt.PIVOT_ROWS.values()) >= VEC_TRIP
    assert sorted(pt.PIVOT_ROWS, key=pt.PIVOT_ROWS.get) == ["negative", "nan", "zero"]
    assert va[pt.PIVOT_ROWS["negative"]] < 0 and np.isnan(va[pt.PIVOT_ROWS["nan"]]) and va[pt.PIVOT_ROWS["zero"]] == 0
    assert cpu_factor(spmv, kind, n, rp, ci, va)[1] == pt.PIVOT_BAD[kind]
    assert cpu_factor(spmv, kind, *pt.pivot_scan_matrix(clean=True))[1] == -1


# ------------------------------------------------------------------------------------------ 2. sptrsv_csr_multi
def _multi_case_is_exact(spmv, case, k, ordered):
    X, B, widest = pt.multi_rhs(case, k)
    assert widest.shape == (k,) and (widest < EXACT_LIMIT).all(), widest      # column by column
    assert np.abs(X).max() == 100 and not np.array_equal(X[:, 0], X[:, k - 1])
    A = spmv.csr_from_arrays(case["n"], case["n"], case["rp"], case["ci"], case["va"])
    try:
        cfg = spmv.SpTRSVConfig(uplo=case["uplo"], diag=case["unit"], ordered=ordered)
        np.testing.assert_array_equal(bits(spmv.sptrsv_cpu_csr_multi(A, B, cfg)), bits(X))
    finally:
        spmv.csr_destroy(A)
    status, level_ptr, _, levels, _ = spmv.sptrsv_levels(case["n"], case["rp"], case["ci"], case["uplo"])
    assert (status, levels) == (0, 2) and np.diff(level_ptr).tolist() == [case["half"]] * 2


@pytest.mark.parametrize("L,uplo,unit", pt.MULTI_CASES)
def test_nine_integer_columns_on_two_wide_levels(spmv, L, uplo, unit):
    case = ed.two_level_triangle(L, uplo, unit)
    assert case["half"] == pt.past_row_cap(L) and pt.trips(case["half"], row_trip(L)) == 2
    assert pt.MULTI_K > 8                                               # the second window of eight
    _multi_case_is_exact(spmv, case, pt.MULTI_K, 0)


@pytest.mark.parametrize("uplo,unit", pt.ORDERED_CASES)
def test_five_columns_for_the_ordered_kernel_past_its_cap(spmv, uplo, unit):
    case = ed.two_level_triangle(1, uplo, unit)
    assert pt.trips(case["half"], row_trip(1)) == 2 and 4 < pt.ORDERED_K <= 8       # the second half of a window
    _multi_case_is_exact(spmv, case, pt.ORDERED_K, 1)


# ------------------------------------------------------------------------------------------ 3. FSAI
@pytest.mark.parametrize("cls,L,order", pt.FSAI_TRIP_CASES)
def test_fsai_trip_shapes(spmv, cls, L, order):
    G = pt.FSAI_ROWS_PER_BLOCK(cls, L)
    n, split, before, after = pt.fsai_trip_shape(cls, L, order)
    deep = order == "deep"
    assert n == 2048 * G + G + 1 + (64 if deep else 0) and split == 2048 * G
    assert pt.row_grid(n, G) == pt.ROW_BLOCKS and pt.trips(n, pt.ROW_BLOCKS * G) == 2
    assert {before, after} == {cls - 1, 1} and (before > after) == (order != "short_first")
    n, rp, ci, va = pt.fsai_trip_matrix(cls, L, order)
    g_rp, g_ci = fc.lower_pattern(n, rp, ci)
    lengths = np.diff(g_rp)
    i = np.arange(n)
    np.testing.assert_array_equal(lengths, np.minimum(i, np.where(i < split, before, after)) + 1)
    assert lengths.max() == cls == fc.class_for(int(lengths.max()))
    assert lengths[split:].tolist() == [after + 1] * (n - split)       # what the second trip holds
    if deep:       # the last whole workgroup of the second trip held rows of the full length in the first
        last = (n - split) // G - 1
        assert last * G >= cls - 1 and (lengths[last * G:(last + 1) * G] == cls).all()
        assert (lengths[split + last * G:split + (last + 1) * G] == 2).all()
    status, bad, got = host_fsai(spmv, n, rp, ci, va)
    assert (status, bad) == (0, -1)
    np.testing.assert_array_equal(got[0], g_rp)
    np.testing.assert_array_equal(got[1], g_ci)
    status, bad, again = host_fsai(spmv, n, rp, ci, pt.rescaled(n, rp, ci, va))
    assert (status, bad) == (0, -1) and not np.array_equal(bits(again[2]), bits(got[2]))


def test_fsai_exact_tier_repeats_one_proved_period(spmv):
    n0, rp0, ci0, va0, L0 = pt.fsai_exact_period()
    assert n0 == sum(pt.FSAI_PERIOD) == 24
    n, rp, ci, va = pt.fsai_exact_matrix()
    rows_per_block = pt.FSAI_ROWS_PER_BLOCK(8, pt.FSAI_EXACT_LANES)
    assert n == 8208 and rows_per_block == 4 and pt.trips(n, pt.ROW_BLOCKS * rows_per_block) == 2
    # the blocks repeat with the period: row r + 24 is row r, its columns 24 further on
    lengths = np.diff(rp)
    np.testing.assert_array_equal(lengths[n0:], lengths[:-n0])
    per = int(rp0[-1])
    np.testing.assert_array_equal(ci[per:], ci[:-per] + n0)
    np.testing.assert_array_equal(bits(va[per:]), bits(va[:-per]))
    np.testing.assert_array_equal(ci[:per], ci0)
    np.testing.assert_array_equal(bits(va[:per]), bits(va0))
    g_rp, g_ci, g = pt.fsai_exact_expected()
    lower = fc.lower_pattern(n, rp, ci)
    np.testing.assert_array_equal(g_rp, lower[0])
    np.testing.assert_array_equal(g_ci, lower[1])
    assert np.diff(g_rp).max() == 6 and fc.class_for(6) == 8
    # G L = I on the period (the whole matrix is its block-diagonal repetition)
    dense = np.zeros((n0, n0))
    dense[fc.rows_of(n0, g_rp[:n0 + 1]), g_ci[:g_rp[n0]]] = g[:g_rp[n0]]
    assert np.array_equal(dense @ L0, np.eye(n0))
    status, bad, got = host_fsai(spmv, n, rp, ci, va)
    assert (status, bad) == (0, -1)
    np.testing.assert_array_equal(bits(got[2]), bits(g))


def test_fsai_structure_defects_sit_past_the_vector_cap(spmv):
    E = spmv.SpMVError
    assert min(pt.FSAI_DEFECT_ROWS.values()) >= VEC_TRIP and max(pt.FSAI_DEFECT_ROWS.values()) < pt.VEC_ROWS
    n, rp, ci, va = pt.fsai_structure_matrix()
    assert n == pt.VEC_ROWS and pt.trips(n + 1, VEC_TRIP) == 2
    status, bad, clean = host_fsai(spmv, n, rp, ci, va)
    assert (status, bad) == (0, -1) and clean[1].size == 2 * n - 1
    want = {"unsorted": E.INVALID_ARGUMENT, "no_diagonal": E.INVALID_ARGUMENT, "wild_column": E.INVALID_FORMAT,
            "long_row": E.INVALID_ARGUMENT}
    for defect, code in want.items():
        m = pt.fsai_structure_matrix(defect)
        assert host_fsai(spmv, *m)[0] == code, defect
        # the one flaw: every other row is the clean matrix's
        r = pt.FSAI_DEFECT_ROWS[defect]
        np.testing.assert_array_equal(np.diff(m[1])[np.arange(n) != r], np.diff(rp)[np.arange(n) != r])
    long_rp, long_ci = pt.fsai_structure_matrix("long_row")[1:3]
    r = pt.FSAI_DEFECT_ROWS["long_row"]
    assert int(np.sum(long_ci[long_rp[r]:long_rp[r + 1]] <= r)) == fc.MAX_ROW + 1
    status, bad, got = host_fsai(spmv, *pt.fsai_structure_matrix("bad_row"))
    assert (status, bad) == (0, pt.FSAI_DEFECT_ROWS["bad_row"])


# ------------------------------------------------------------------------------------------ 4. AMG V-cycle
def test_the_fast_prover_is_the_fraction_prover():
    from test_gpu_amg import EXACT
    admitted = 0
    for n, coarsest in EXACT:                                           # the dense coarsest level
        for sweeps in (1, 2):
            r = ac.exact_rhs(n)
            want, width = ac.prove_vcycle(n, coarsest, r, 0.5, sweeps)
            got, got_width = pt.prove_vcycle_fast(n, coarsest, r, 0.5, sweeps, sweeps)
            assert (got is None) == (want is None), (n, sweeps, width, got_width)
            if want is not None:
                admitted += 1
                assert got_width == width
                np.testing.assert_array_equal(bits(got), bits(want))
                again, again_width = pt.prove_vcycle_fractions(n, coarsest, r, 0.5, sweeps, sweeps)
                assert again_width == width
                np.testing.assert_array_equal(bits(again), bits(want))
    assert admitted >= 3
    r = ac.exact_rhs(56)
    for pre, coarse, post in pt.AMG_TWIN_CHECKS:                        # the Jacobi-solved coarsest level
        want, width = pt.prove_vcycle_fractions(56, 28, r, pt.AMG_OMEGA, pre, post, coarse)
        got, got_width = pt.prove_vcycle_fast(56, 28, r, pt.AMG_OMEGA, pre, post, coarse)
        assert want is not None and got is not None, (pre, coarse, post, width, got_width)
        assert got_width == width
        np.testing.assert_array_equal(bits(got), bits(want))
    # both refuse a right-hand side too wide for fp32
    wide = r * np.float32(1 << 20)
    assert pt.prove_vcycle_fast(56, 28, wide, pt.AMG_OMEGA, 1, 1, 4)[0] is None
    assert pt.prove_vcycle_fractions(56, 28, wide, pt.AMG_OMEGA, 1, 1, 4)[0] is None


@pytest.mark.parametrize("name", list(pt.AMG_CASES))
def test_every_vcycle_case_is_admitted_and_passes_its_caps(name):
    n, lanes, sweep_counts = pt.AMG_CASES[name]
    coarse = n // 2
    assert n % 2 == 0 and coarse > ac.DENSE_ROWS                        # Jacobi-solved: no dense inverse
    if lanes is not None:
        assert pt.trips(n, row_trip(lanes)) == 3 and pt.trips(coarse, row_trip(lanes)) == 2
        assert pt.row_grid(coarse, 256 // lanes) == pt.ROW_BLOCKS      # the sweep of level 1, the restriction of level 0
        assert coarse - row_trip(lanes) == (5 if lanes == 64 else 33)
    else:
        assert coarse == pt.VEC_ROWS and pt.trips(n, VEC_TRIP) == 3 and pt.trips(coarse, VEC_TRIP) == 2
    r = ac.exact_rhs(n)
    for pre, coarse_sweeps, post in sweep_counts:
        z, width = pt.prove_vcycle_fast(n, coarse, r, pt.AMG_OMEGA, pre, post, coarse_sweeps)
        print(f"{name}: n = {n}, (pre, coarse, post) = {(pre, coarse_sweeps, post)}: " +
              (f"{width} bits" if z is not None else f"not admitted ({width})"))
        assert z is not None, (name, pre, coarse_sweeps, post, width)
        assert width <= 24 and np.abs(z).max() > 0


# ------------------------------------------------------------------------------------------ 5. AMG setup
def test_the_setup_shapes_sit_at_and_past_their_caps(spmv):
    n = pt.MIS_CAP_GRID ** 2
    assert n == 9216 and pt.trips(n, 256 // 64) > pt.ROW_BLOCKS == pt.row_grid(n, 256 // 64)   # Scratch::partial is full
    assert pt.trips(n, row_trip(64)) == 2
    n = pt.MIS_L8_GRID ** 2
    assert row_trip(8) < n <= row_trip(8) + 1024 and pt.row_grid(n, 256 // 8) == pt.ROW_BLOCKS
    assert pt.trips(pt.VEC_ROWS + 1, VEC_TRIP) == 2 and pt.vec_grid(pt.VEC_ROWS) == pt.VEC_BLOCKS
    assert VEC_TRIP <= pt.SETUP_BAD_ROW < pt.VEC_ROWS and pt.SETUP_LAST_PARTIAL_ROW // pt.BLOCK == pt.VEC_BLOCKS - 1
    # the definition on the long path: it aggregates, and the coarse level is still past the dense solve's limit
    nrows, rp, ci, va = pt.tridiagonal(pt.VEC_ROWS)
    A = spmv.csr_from_arrays(nrows, nrows, rp, ci, va)
    status, agg, count, rounds = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
    spmv.csr_destroy(A)
    assert status == 0 and agg.min() >= 0 and agg.max() == count - 1 and rounds >= 1
    assert ac.DENSE_ROWS < count < nrows
