"""Block IC(0), the block triangular solves and cg_solve_bsr_ic (include/spmv/bsr_factor.h, include/spmv/cg.h) without a
GPU: names and signatures; bsr_ic0_cpu and sptrsv_cpu_bsr against the numpy restatements of tests/bsr_ic_cases.py bit
for bit (every block size, every ragged tail, denormal- and huge-scaled blocks, a non-positive pivot); the exact
family proved in exact rationals; every rejection of every entry point in its documented order, the device entry points
with fake device addresses that must never be dereferenced; block IC(0) needing at most half of block-Jacobi's steps
in the fp32 restatement; the selection rules of the float parity systems; and the sanitized caller."""
import os
import re
import subprocess

import numpy as np
import pytest

import bsr_ic_cases as ic
from conftest import ROOT

NAMES = ("bsr_ic0_cpu", "bsr_ic0", "bsr_ic0_async", "sptrsv_cpu_bsr", "sptrsv_bsr", "sptrsv_bsr_async",
         "sptrsv_analyze_bsr", "cg_solve_bsr_ic")
OK, DIMENSION, FORMAT, ARGUMENT = 0, -1, -5, -8
FAKE_RP, FAKE_CI, FAKE_VA, FAKE_B, FAKE_X, FAKE_F = 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000


def _bsr(spmv, n, b, brp, bc, bv):
    return spmv.bsr_from_arrays(n, n, b, brp, bc, bv)


def _cpu_factor(spmv, n, b, brp, bc, bv):
    A = _bsr(spmv, n, b, brp, bc, bv)
    f, bad = spmv.bsr_ic0_cpu(A)
    spmv.bsr_destroy(A)
    return f, bad


# ---- names ---------------------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)
    cxx = open(os.path.join(ROOT, "include", "spmv", "bsr_factor.h")).read() + \
        open(os.path.join(ROOT, "include", "spmv", "cg.h")).read()
    for name in NAMES:
        c_name = "spmv_c_" + name
        assert c_name in declared and hasattr(spmv.lib(), c_name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    for text in ("int spmv_c_bsr_ic0_cpu(const spmv_c_bsr* A, float* f_values, int* bad_pivot);",
                 "int spmv_c_bsr_ic0(const spmv_c_bsr* A, float* d_f_values, spmv_c_ic0_result* out);",
                 "int spmv_c_bsr_ic0_async(const spmv_c_bsr* A, float* d_f_values, void* hip_stream);",
                 "int spmv_c_sptrsv_cpu_bsr(const spmv_c_bsr* F, const float* b, float* x, "
                 "const spmv_c_sptrsv_config* config);",
                 "int spmv_c_sptrsv_analyze_bsr(const spmv_c_bsr* A, int uplo, spmv_c_sptrsv_result* out);",
                 "int spmv_c_cg_solve_bsr_ic(const spmv_c_bsr* A, const spmv_c_bsr* F, const float* d_b, float* d_x,"):
        assert text in header, text
    assert "inverse of the diagonal block is stored" in cxx.lower()


# ---- the host twins against the restatements -------------------------------------------------------------------
@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_bsr_ic0_cpu_is_the_restatement_bit_for_bit(spmv, b):
    for name, n, brp, bc, bv in ic.float_family(b):
        f, bad = _cpu_factor(spmv, n, b, brp, bc, bv)
        want, want_bad = ic.ic0(n, b, brp, bc, bv)
        assert bad == want_bad == -1, name
        ic.assert_bits(f, ic.factor_array(want, b), name)
        # symmetric diagonal blocks, zero padding, and really a factor: L L^T = A on the stored pattern where nothing
        # was dropped is covered by the exact family; here the solves must reduce the residual
        F = np.asarray(f, np.float32).reshape(-1, b, b)
        diag = ic.diagonal_positions(brp, bc)
        assert np.array_equal(F[diag], np.transpose(F[diag], (0, 2, 1))), name
        cut = len(brp) - 1
        size = n - (cut - 1) * b
        assert not F[diag[-1]][size:, :].any() and not F[diag[-1]][:, size:].any(), name


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
@pytest.mark.parametrize("scale", (2.0 ** -130, 2.0 ** 100))
def test_denormal_and_huge_scaled_blocks(spmv, b, scale):
    nodes, pairs = ic.grid_pattern("2d9", 3)
    n, brp, bc, bv = ic.laplacian_bsr(nodes, pairs, b, nodes * b - (b - 1), seed=5)
    bv = (bv.astype(np.float64) * scale).astype(np.float32)
    f, bad = _cpu_factor(spmv, n, b, brp, bc, bv)
    want, want_bad = ic.ic0(n, b, brp, bc, bv)
    assert bad == want_bad
    got, ref = ic.bits(f), ic.bits(ic.factor_array(want, b))
    nan = np.isnan(f) & np.isnan(ic.factor_array(want, b))        # NaN payloads are not part of the contract
    assert np.array_equal(got[~nan], ref[~nan]), (b, scale)


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_a_non_positive_pivot_is_reported_and_is_not_an_error(spmv, b):
    nodes, pairs = ic.grid_pattern("2d9", 3)
    n, brp, bc, bv = ic.laplacian_bsr(nodes, pairs, b, seed=6)
    diag = ic.diagonal_positions(brp, bc)
    blocks = bv.reshape(-1, b, b).copy()
    blocks[diag[4], b - 1, b - 1] = -1.0                           # block row 4 meets a negative pivot
    bv = blocks.reshape(-1)
    f, bad = _cpu_factor(spmv, n, b, brp, bc, bv)
    want, want_bad = ic.ic0(n, b, brp, bc, bv)
    assert bad == want_bad == 4
    ref = ic.factor_array(want, b)
    nan = np.isnan(f)
    assert np.array_equal(nan, np.isnan(ref)) and nan.any()
    assert np.array_equal(ic.bits(f)[~nan], ic.bits(ref)[~nan])
    # block rows above the bad one are untouched by it
    first = int(brp[4]) * b * b
    assert not nan[:first].any()


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_sptrsv_cpu_bsr_is_the_restatement_bit_for_bit(spmv, b):
    rng = np.random.default_rng(b)
    family = ic.float_family(b)
    for name, n, brp, bc, bv in family[:3] + family[-2:]:
        f, _ = _cpu_factor(spmv, n, b, brp, bc, bv)
        F = _bsr(spmv, n, b, brp, bc, f)
        rhs = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for uplo in (ic.LOWER, ic.UPPER):
            for unit in (0, 1):
                cfg = spmv.SpTRSVConfig(uplo=uplo, diag=unit, ordered=1)
                status, x = spmv.sptrsv_cpu_bsr(F, rhs, None, cfg)
                want = ic.solve(n, b, brp, bc, f, rhs, uplo, bool(unit))
                assert status == OK
                ic.assert_bits(x, want, (name, uplo, unit))
                inplace = rhs.copy()
                status, x2 = spmv.sptrsv_cpu_bsr(F, inplace, inplace, cfg)
                assert status == OK
                ic.assert_bits(x2, want, (name, uplo, unit, "in place"))
        spmv.bsr_destroy(F)


# ---- the exact family ------------------------------------------------------------------------------------------
def _exact_cases(b):
    out = [("chain", ic.exact_forest(1, 5, b)), ("forest", ic.exact_forest(3, 3, b)),
           ("block diagonal", ic.exact_forest(4, 1, b)), ("arrow", ic.exact_arrow(4, b))]
    for cut in range(1, b):
        out.append(("chain cut %d" % cut, ic.exact_forest(1, 4, b, 4 * b - cut)))
        out.append(("arrow cut %d" % cut, ic.exact_arrow(3, b, 4 * b - cut)))
    return out


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_the_exact_family_is_exact(spmv, b):
    for name, s in _exact_cases(b):
        n, brp, bc, bv = s["n"], s["brp"], s["bc"], s["bv"]
        # every intermediate of the definition is representable, so the rounded program is the exact one
        before = ic.ExactOps.count
        exact, bad = ic.ic0(n, b, brp, bc, bv, ic.ExactOps)
        assert bad == -1 and ic.ExactOps.count > before, name
        ic.assert_bits(ic.factor_array(exact, b), s["fv"], name + " exact program")
        f, bad = _cpu_factor(spmv, n, b, brp, bc, bv)
        assert bad == -1
        # (a zero of V below its diagonal is -(+0.0) / l_ii = -0.0 by the definition: the sign of a zero is the one
        # thing the rationals do not carry, so zeros are compared as zeros)
        ic.assert_bits(f + np.float32(0.0), s["fv"], name + " library")
        ic.assert_bits(f, ic.factor_array(ic.ic0(n, b, brp, bc, bv)[0], b), name + " library against the restatement")
        # the solves: every partial sum in any order is representable
        x, rhs = ic.exact_solution(s)
        assert ic.solve_partial_sum_bound(s, x) < 2.0 ** 24, name
        F = _bsr(spmv, n, b, brp, bc, f)
        status, y = spmv.sptrsv_cpu_bsr(F, rhs, None, spmv.SpTRSVConfig(uplo=ic.LOWER, ordered=1))
        status2, got = spmv.sptrsv_cpu_bsr(F, y, None, spmv.SpTRSVConfig(uplo=ic.UPPER, ordered=1))
        spmv.bsr_destroy(F)
        assert status == status2 == OK
        ic.assert_bits(got, x + np.float32(0.0), name + " L^-T L^-1 A x")
        # CG from x0 = 0 with the exact factor: one step, alpha = 1, r = 0, x = x*
        A64 = ic.expand(n, b, brp, bc, bv)
        xs, it, conv, brk, rel = ic.restate_cg(A64, rhs, 1e-6, ic.ic_apply(n, b, brp, bc, f))
        if not rhs.any():
            continue
        assert (it, conv, brk, rel) == (1, True, False, 0.0), name
        ic.assert_bits(xs, x + np.float32(0.0), name + " one CG step")


# ---- rejections ------------------------------------------------------------------------------------------------
def _small(b=2):
    nodes, pairs = ic.grid_pattern("2d9", 3)
    return ic.laplacian_bsr(nodes, pairs, b, seed=2)


def test_each_rejection_of_bsr_ic0_cpu(spmv):
    n, brp, bc, bv = _small()
    lib = spmv.lib()
    out = np.zeros(bv.size, np.float32)
    A = _bsr(spmv, n, 2, brp, bc, bv)
    assert lib.spmv_c_bsr_ic0_cpu(None, spmv._np_ptr(out), None) == ARGUMENT
    assert lib.spmv_c_bsr_ic0_cpu(A, None, None) == ARGUMENT
    A.contents.num_cols += 2
    A.contents.num_block_cols += 1
    assert lib.spmv_c_bsr_ic0_cpu(A, spmv._np_ptr(out), None) == DIMENSION
    A.contents.num_cols -= 2
    A.contents.num_block_cols -= 1
    A.contents.num_block_rows += 1
    assert lib.spmv_c_bsr_ic0_cpu(A, spmv._np_ptr(out), None) == FORMAT
    A.contents.num_block_rows -= 1
    # a partial overlap with A's own values
    base = spmv.ctypes.cast(A.contents.values, spmv.c_void_p).value
    assert lib.spmv_c_bsr_ic0_cpu(A, spmv.c_void_p(base + 4), None) == ARGUMENT
    assert not out.any()
    spmv.bsr_destroy(A)
    E = spmv.bsr_create(0, 0, 2, 0)
    pivot = spmv.c_int32(7)
    assert lib.spmv_c_bsr_ic0_cpu(E, spmv._np_ptr(out), spmv.byref(pivot)) == OK and pivot.value == -1
    spmv.bsr_destroy(E)

    def status_of(brp2, bc2, bv2):
        M = _bsr(spmv, n, 2, brp2, bc2, bv2)
        status = lib.spmv_c_bsr_ic0_cpu(M, spmv._np_ptr(out), None)
        spmv.bsr_destroy(M)
        return status

    bad_ptr = brp.copy()
    bad_ptr[3] = bad_ptr[2] - 1
    assert status_of(bad_ptr, bc, bv) == FORMAT
    bad_col = bc.copy()
    bad_col[1] = len(brp) - 1
    assert status_of(brp, bad_col, bv) == FORMAT
    swapped = bc.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert status_of(brp, swapped, bv) == ARGUMENT                  # not strictly ascending
    # block row 0 without its diagonal block: its first block column renamed to an unused later one
    blocks = bv.reshape(-1, 2, 2)
    keep = np.ones(bc.size, bool)
    keep[0] = False
    brp_m = brp.copy()
    brp_m[1:] -= 1
    assert status_of(brp_m, bc[keep], blocks[keep].reshape(-1)) == ARGUMENT     # no diagonal block
    # one-sided: drop (0, J) but keep (J, 0)
    keep = np.ones(bc.size, bool)
    keep[1] = False
    assert status_of(brp_m, bc[keep], blocks[keep].reshape(-1)) == ARGUMENT
    assert not out.any()


def test_each_rejection_of_sptrsv_cpu_bsr(spmv):
    n, brp, bc, bv = _small()
    lib = spmv.lib()
    F = _bsr(spmv, n, 2, brp, bc, bv)
    rhs, x = np.ones(n, np.float32), np.full(n, 9.0, np.float32)
    p = spmv._np_ptr
    assert lib.spmv_c_sptrsv_cpu_bsr(None, p(rhs), p(x), None) == ARGUMENT
    assert lib.spmv_c_sptrsv_cpu_bsr(F, None, p(x), None) == ARGUMENT
    assert lib.spmv_c_sptrsv_cpu_bsr(F, p(rhs), None, None) == ARGUMENT
    for field, value in (("uplo", 2), ("diag", 2), ("ordered", 2)):
        assert lib.spmv_c_sptrsv_cpu_bsr(F, p(rhs), p(x), spmv.byref(spmv.SpTRSVConfig(**{field: value}))) == ARGUMENT
    both = np.ones(n + 1, np.float32)
    assert lib.spmv_c_sptrsv_cpu_bsr(F, p(both), spmv.c_void_p(both.ctypes.data + 4), None) == ARGUMENT
    spmv.bsr_destroy(F)
    # NON_UNIT finds the diagonal block in ascending block columns; UNIT picks the triangle's blocks by their column
    swapped = bc.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    M = _bsr(spmv, n, 2, brp, swapped, bv)
    assert lib.spmv_c_sptrsv_cpu_bsr(M, p(rhs), p(x), None) == ARGUMENT and (x == 9.0).all()
    assert lib.spmv_c_sptrsv_cpu_bsr(M, p(rhs), p(x), spmv.byref(spmv.SpTRSVConfig(diag=1))) == OK
    spmv.bsr_destroy(M)
    x[:] = 9.0
    keep = np.ones(bc.size, bool)
    keep[0] = False
    brp_m = brp.copy()
    brp_m[1:] -= 1
    M = _bsr(spmv, n, 2, brp_m, bc[keep], bv.reshape(-1, 2, 2)[keep].reshape(-1))
    assert lib.spmv_c_sptrsv_cpu_bsr(M, p(rhs), p(x), None) == ARGUMENT               # NON_UNIT needs the diagonal
    assert lib.spmv_c_sptrsv_cpu_bsr(M, p(rhs), p(x), spmv.byref(spmv.SpTRSVConfig(diag=1))) == OK
    spmv.bsr_destroy(M)


def test_the_device_entry_points_reject_before_they_touch_the_device(spmv):
    """every rejection that needs no device, in the documented order, on fake addresses"""
    b, nbr, blocks = 2, 4, 10
    n = nbr * b
    wrap = lambda rows=n, cols=n, rp=FAKE_RP, ci=FAKE_CI, va=FAKE_VA: spmv.bsr_wrap_device(rows, cols, b, blocks, rp, ci,
                                                                                          va)
    A = wrap()
    # bsr_ic0 / bsr_ic0_async
    for call in (lambda M, f: spmv.bsr_ic0(M, f).error_code, lambda M, f: spmv.bsr_ic0_async(M, f)):
        assert call(None, FAKE_F) == ARGUMENT
        assert call(A, None) == ARGUMENT
        M = wrap(cols=n + 2)
        assert call(M, FAKE_F) == DIMENSION
        spmv.bsr_destroy(M)
        M = spmv.bsr_wrap_device(0, 0, b, 0, None, None, None)
        assert call(M, FAKE_F) == OK
        spmv.bsr_destroy(M)
        M = wrap(rp=None)
        assert call(M, FAKE_F) == FORMAT
        spmv.bsr_destroy(M)
        M = wrap(va=None)
        assert call(M, FAKE_F) == FORMAT
        spmv.bsr_destroy(M)
        assert call(A, FAKE_VA + 4) == ARGUMENT                   # a partial overlap
        assert call(A, FAKE_VA + 4 * blocks * b * b - 4) == ARGUMENT
    # sptrsv_bsr / sptrsv_bsr_async / sptrsv_analyze_bsr
    for call in (lambda M, bb, xx, c=None: spmv.sptrsv_bsr(M, bb, xx, c).error_code,
                 lambda M, bb, xx, c=None: spmv.sptrsv_bsr_async(M, bb, xx, c)):
        assert call(None, FAKE_B, FAKE_X) == ARGUMENT
        assert call(A, None, FAKE_X) == ARGUMENT
        assert call(A, FAKE_B, None) == ARGUMENT
        M = wrap(cols=n + 2)
        assert call(M, FAKE_B, FAKE_X) == DIMENSION
        spmv.bsr_destroy(M)
        M = spmv.bsr_wrap_device(0, 0, b, 0, None, None, None)
        assert call(M, FAKE_B, FAKE_X) == OK
        spmv.bsr_destroy(M)
        M = wrap(ci=None)
        assert call(M, FAKE_B, FAKE_X) == FORMAT
        spmv.bsr_destroy(M)
        for field in ("uplo", "diag", "ordered"):
            assert call(A, FAKE_B, FAKE_X, spmv.SpTRSVConfig(**{field: 2})) == ARGUMENT
        assert call(A, FAKE_B, FAKE_B + 4) == ARGUMENT
    assert spmv.sptrsv_analyze_bsr(None, 0).error_code == ARGUMENT
    M = wrap(cols=n + 2)
    assert spmv.sptrsv_analyze_bsr(M, 0).error_code == DIMENSION
    spmv.bsr_destroy(M)
    M = wrap(rp=None)
    assert spmv.sptrsv_analyze_bsr(M, 0).error_code == FORMAT
    spmv.bsr_destroy(M)
    assert spmv.sptrsv_analyze_bsr(A, 2).error_code == ARGUMENT
    # cg_solve_bsr_ic: cg_solve_bsr's checks first, the preconditioner not read, then F
    F = wrap(va=FAKE_F)
    solve = lambda *a, **k: spmv.cg_solve_bsr_ic(*a, **k).error_code
    assert solve(None, F, FAKE_B, FAKE_X) == ARGUMENT
    assert solve(A, F, None, FAKE_X) == ARGUMENT
    M = wrap(cols=n + 2)
    assert solve(M, F, FAKE_B, FAKE_X) == DIMENSION
    spmv.bsr_destroy(M)
    M = wrap(rp=None)
    assert solve(M, F, FAKE_B, FAKE_X) == FORMAT
    spmv.bsr_destroy(M)
    assert solve(A, F, FAKE_B, FAKE_X, spmv.CGConfig(tolerance=-1.0)) == ARGUMENT
    assert solve(A, F, FAKE_B, FAKE_X, spmv.CGConfig(engine=1)) == ARGUMENT
    assert solve(A, F, FAKE_B, FAKE_B + 4) == ARGUMENT
    assert solve(A, None, FAKE_B, FAKE_X, spmv.CGConfig(preconditioner=77, engine=0)) == ARGUMENT    # null F, not 77
    M = wrap(rows=n + 2, cols=n + 2)
    assert solve(A, M, FAKE_B, FAKE_X, spmv.CGConfig(preconditioner=77, engine=0)) == DIMENSION
    spmv.bsr_destroy(M)
    M = spmv.bsr_wrap_device(n, n, 4, blocks, FAKE_RP, FAKE_CI, FAKE_F)
    assert solve(A, M, FAKE_B, FAKE_X) == DIMENSION                  # another block_dim
    spmv.bsr_destroy(M)
    M = wrap(va=None)
    assert solve(A, M, FAKE_B, FAKE_X) == FORMAT
    spmv.bsr_destroy(M)
    E = spmv.bsr_wrap_device(0, 0, b, 0, None, None, None)
    res = spmv.cg_solve_bsr_ic(E, None, FAKE_B, FAKE_X)
    assert (res.error_code, res.converged) == (OK, 1)
    for M in (A, F, E):
        spmv.bsr_destroy(M)


# ---- what the factor is for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", (2, 3, 4))
def test_block_ic0_needs_at_most_half_of_block_jacobis_steps(spmv, b):
    n, brp, bc, bv = ic.laplacian_system(16, b)
    rhs = np.random.default_rng(11).uniform(-1.0, 1.0, n).astype(np.float32)
    A64 = ic.expand(n, b, brp, bc, bv)
    f, bad = _cpu_factor(spmv, n, b, brp, bc, bv)
    assert bad == -1
    _, it_ic, conv_ic, _, _ = ic.restate_cg(A64, rhs, 1e-6, ic.ic_apply(n, b, brp, bc, f))
    _, it_bj, conv_bj, _, _ = ic.restate_cg(A64, rhs, 1e-6, ic.block_jacobi_apply(n, b, brp, bc, bv))
    print("b", b, "n", n, "block IC(0)", it_ic, "BLOCK_JACOBI", it_bj)
    assert conv_ic and conv_bj
    assert 2 * it_ic <= it_bj, (b, it_ic, it_bj)


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_the_float_parity_systems_meet_the_selection_rules(spmv, b):
    """cg_bsr_cases.py's two rules for a system whose end state two correct realisations share: the restatement's last
    residual lies at least 5 % below the tolerance and the one before at least 5 % above it (stop_margin), and the five
    other realisations of reference_spread (the product summed in fp32, three with roundoff-sized noise on q, and the
    product in the lane-group kernel's documented order) end on the same step within a quarter of the 1 % the device
    is allowed."""
    for name, n, brp, bc, bv, rhs, tol in ic.parity_systems(b):
        A64 = ic.expand(n, b, brp, bc, bv)
        f, _ = _cpu_factor(spmv, n, b, brp, bc, bv)
        apply = ic.ic_apply(n, b, brp, bc, f)
        x, it, conv, brk, rel = ic.restate_cg(A64, rhs, tol, apply)
        assert conv and not brk and it >= 2, name
        before = ic.restate_cg(A64, rhs, 0.0, apply, max_iter=it - 1)[4]
        t = float(np.float32(tol))
        margin = min(1.0 - rel / t, before / t - 1.0)
        spread, steps = 0.0, 0
        for product in ic.other_products(n, b, brp, bc, bv):
            other = ic.restate_cg(A64, rhs, tol, apply, spmv=product)
            spread = max(spread, abs(other[4] - rel) / rel)
            steps = max(steps, abs(other[1] - it))
        print(name, "steps", it, "margin", margin, "spread", spread)
        assert margin >= 0.05, (name, margin)
        assert steps == 0 and spread <= 0.0025, (name, steps, spread)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_the_host_routines_are_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-bsr-ic builds tests/cpp/bin/bsr_ic_host_sanitized (csrc/bsr_tri_host.cpp and the
    BSR host files it needs, with tests/cpp/bsr_ic_host_sanitized.cpp, under AddressSanitizer + UBSan); any sanitizer
    report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-bsr-ic"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "bsr_ic_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
