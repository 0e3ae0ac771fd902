"""cg_solve_bsr and the block-Jacobi routines (include/spmv/cg.h, include/spmv/bsr.h) without a GPU: names and
signatures; bsr_diag_inverse_cpu and bsr_diag_apply_cpu against their numpy restatements bit for bit; each rejection;
the Kronecker lift of tests/cg_bsr_cases.py proved in exact rationals; BLOCK_JACOBI needing fewer steps than JACOBI in
the restatement; the argument rejections of the device entry points in their documented order with fake device
addresses that must never be dereferenced; and the sanitized caller."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import cg_bsr_cases as cc
import exact_data as ed
from conftest import ROOT

NAMES = ("cg_solve_bsr", "bsr_diag_inverse_cpu", "bsr_diag_inverse_gpu", "bsr_diag_apply_cpu", "bsr_diag_apply")
OK, DIMENSION, FORMAT, ARGUMENT = 0, -1, -5, -8
FAKE_RP, FAKE_CI, FAKE_VA, FAKE_B, FAKE_X = 0x300000, 0x400000, 0x500000, 0x600000, 0x700000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what=""):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def _bsr(spmv, n, b, rp, ci, va):
    """bsr_from_csr_cpu of CSR arrays with ascending columns"""
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    B = spmv.bsr_create(3, 3, 2, 1)
    assert spmv.bsr_from_csr_cpu(B, A, b) == 0
    spmv.csr_destroy(A)
    return B


def _dense_blocks_csr(n, b, blocks):
    """CSR arrays of a block-diagonal matrix from [nb, b, b] blocks (every position inside the matrix stored)"""
    nb = blocks.shape[0]
    rows = (np.arange(nb)[:, None, None] * b + np.arange(b)[None, :, None] + np.zeros((1, 1, b), np.int64)).ravel()
    cols = (np.arange(nb)[:, None, None] * b + np.zeros((1, b, 1), np.int64) + np.arange(b)[None, None, :]).ravel()
    vals = blocks.astype(np.float32).ravel()
    keep = (rows < n) & (cols < n)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp, cols.astype(np.int32), vals


def _random_spd_blocks(rng, nb, b, scale=1.0):
    Q = rng.uniform(-1.0, 1.0, size=(nb, b, b))
    D = np.einsum("eki,ekj->eij", Q, Q) + 0.1 * np.eye(b)[None]
    return (0.5 * (D + np.einsum("eij->eji", D)) * scale).astype(np.float32)


# ---- names ---------------------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)
    cxx = open(os.path.join(ROOT, "include", "spmv", "bsr.h")).read() + \
        open(os.path.join(ROOT, "include", "spmv", "cg.h")).read()
    for name in NAMES:
        c_name = "spmv_c_" + name
        assert c_name in declared and hasattr(spmv.lib(), c_name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert re.search(r"BLOCK_JACOBI\s*=\s*2", cxx)
    # the C signatures, as spmv_c.h states them
    for text in ("int spmv_c_bsr_diag_inverse_cpu(const spmv_c_bsr* A, float* inv);",
                 "int spmv_c_bsr_diag_inverse_gpu(const spmv_c_bsr* A, float* d_inv);",
                 "void spmv_c_bsr_diag_apply_cpu(const spmv_c_bsr* A, const float* inv, const float* r, float* z);",
                 "int spmv_c_bsr_diag_apply(const spmv_c_bsr* A, const float* d_inv, const float* d_r, float* d_z);",
                 "int spmv_c_cg_solve_bsr(const spmv_c_bsr* A, const float* d_b, float* d_x, "
                 "const spmv_c_cg_config* config,"):
        assert text in header, text


# ---- the host twins against the restatements -----------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -70, 2.0 ** 60], ids=["unit", "tiny", "huge"])
@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_inverse_and_apply_equal_the_restatements_bit_for_bit(spmv, b, scale):
    """Sizes with every ragged tail of the last block; 2^-70-scaled blocks have denormal entries next to normal ones and
    inverses that overflow fp32, 2^60-scaled ones inverses that are denormal or zero in fp32."""
    rng = np.random.default_rng([b, 100 + int(np.log2(scale))])
    for tail in range(b):
        nb = 37
        n = nb * b - tail
        blocks = _random_spd_blocks(rng, nb, b, scale)
        if scale < 1.0:
            blocks[::3] *= np.float32(2.0 ** -60)                    # entries below 2^-126: denormals
        B = _bsr(spmv, n, b, *_dense_blocks_csr(n, b, blocks))
        status, inv = spmv.bsr_diag_inverse_cpu(B)
        want, ok = cc.restate_inverse(n, b, blocks)
        assert status == OK and ok.all(), (b, tail, scale)
        assert_bits(inv, want, (b, tail, scale))
        shaped = inv.reshape(nb, b, b)
        assert_bits(shaped, np.swapaxes(shaped, 1, 2), "symmetric bit for bit")
        if tail:                                                      # the rows and columns outside the matrix are +0.0f
            assert not bits(shaped[-1, b - tail:, :]).any() and not bits(shaped[-1, :, b - tail:]).any()
        finite = np.where(np.isfinite(inv), inv, np.float32(1.0))     # the apply on finite factors, wide-range r
        r = (rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-10, 10, n)).astype(np.float32)
        r[::7] = 0.0
        assert_bits(spmv.bsr_diag_apply_cpu(B, finite, r), cc.restate_apply(n, b, finite, r), (b, tail, scale))
        spmv.bsr_destroy(B)


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_only_the_lower_triangle_is_read(spmv, b):
    rng = np.random.default_rng(b)
    nb, n = 11, 11 * b
    blocks = _random_spd_blocks(rng, nb, b)
    B = _bsr(spmv, n, b, *_dense_blocks_csr(n, b, blocks))
    _, want = spmv.bsr_diag_inverse_cpu(B)
    spmv.bsr_destroy(B)
    upper = np.triu(np.ones((b, b), bool), 1)
    blocks[:, upper] = np.nan
    B = _bsr(spmv, n, b, *_dense_blocks_csr(n, b, blocks))
    status, got = spmv.bsr_diag_inverse_cpu(B)
    spmv.bsr_destroy(B)
    assert status == OK
    assert_bits(got, want)


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_each_rejection_of_the_inverse(spmv, b):
    rng = np.random.default_rng(b + 100)
    nb, n = 9, 9 * b - 1
    good = _random_spd_blocks(rng, nb, b)

    def status_of(blocks, drop=None):
        rp, ci, va = _dense_blocks_csr(n, b, blocks)
        if drop is not None:                                          # block row `drop` keeps an off-diagonal block only
            rows = np.repeat(np.arange(n), np.diff(rp))
            other = (drop + 1) % nb
            ci = np.where(rows // b == drop, ci % b + other * b, ci).astype(np.int32)
            keep = ci < n
            rows, ci, va = rows[keep], ci[keep], va[keep]
            rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
        B = _bsr(spmv, n, b, rp, ci, va)
        status, _ = spmv.bsr_diag_inverse_cpu(B)
        spmv.bsr_destroy(B)
        return status

    assert status_of(good) == OK
    assert status_of(good, drop=4) == ARGUMENT                        # no stored diagonal block
    for at in (0, b - 1):
        for value in (0.0, -1.0, np.nan, np.inf):
            bad = good.copy()
            bad[3, at, at] = value                                    # zero, negative, NaN, Inf pivot
            assert status_of(bad) == ARGUMENT, (at, value)
    bad = good.copy()
    bad[5, b - 1, 0] = np.nan                                         # a NaN below the diagonal reaches a pivot
    assert status_of(bad) == ARGUMENT
    bad = good.copy()
    bad[-1, b - 1, b - 1] = -1.0                                      # outside the matrix (n = nb * b - 1): not read
    assert status_of(bad) == OK
    # argument checks: null, not square, missing host arrays
    assert spmv.lib().spmv_c_bsr_diag_inverse_cpu(None, None) == ARGUMENT
    W = spmv.bsr_wrap_device(8, 6, 2, 5, FAKE_RP, FAKE_CI, FAKE_VA)
    inv = np.zeros(64, np.float32)
    assert spmv.lib().spmv_c_bsr_diag_inverse_cpu(W, None) == ARGUMENT
    assert spmv.lib().spmv_c_bsr_diag_inverse_cpu(W, inv.ctypes.data) == DIMENSION
    spmv.bsr_destroy(W)
    W = spmv.bsr_wrap_device(8, 8, 2, 5, FAKE_RP, FAKE_CI, FAKE_VA)  # square, but no host arrays
    assert spmv.lib().spmv_c_bsr_diag_inverse_cpu(W, inv.ctypes.data) == FORMAT
    spmv.bsr_destroy(W)
    assert not inv.any()


# ---- the lift, in exact rationals ----------------------------------------------------------------------------
def _fraction_vector(values):
    return np.array([Fraction(float(v)) for v in values], dtype=object)


def _is_float32(values):
    return all(Fraction(float(np.float32(float(v)))) == v for v in values)


def _check_exact_scaled(rp, ci, va, p):
    """check_exact in units of p's last bit: p scaled by the power of two that makes every entry an integer"""
    k = 0
    while any((v * (1 << k)).denominator != 1 for v in p):
        k += 1
        assert k < 64
    scaled = np.array([float(v * (1 << k)) for v in p], np.float32)
    ed.check_exact(rp, ci, va, scaled)
    return int(ed.row_abs_sums(rp, ci, va, scaled).max())


@pytest.mark.parametrize("identity", [False, True], ids=["K", "I"])
@pytest.mark.parametrize("n0,L", cc.SMALL_LIFTS)
@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_the_lift_ends_in_two_exact_steps(spmv, b, n0, L, identity):
    """cg.h's iteration on A = A0 (x) K, b = b0 (x) w with M = the block diagonal (K) or M = I / diag(A) (K = I), in
    Fractions: alpha = 2, 2, beta = 1/2, r2 = 0, x1 and x2 the stated lifts, every entry of every vector an fp32 value,
    every p inside check_exact's rule, and the host twin's inverse of d K equal to K^-1 / d to the bit."""
    s = cc.lifted_system(n0, L, b, identity)
    n = s["n"]
    rp, ci, va = cc.bsr_to_csr_arrays(n, b, s["brp"], s["bc"], s["bv"])
    B = spmv.bsr_from_arrays(n, n, b, s["brp"], s["bc"], s["bv"])
    status, inv = spmv.bsr_diag_inverse_cpu(B)
    assert status == OK
    assert_bits(inv, s["inv"], "the inverse of d K")
    Ki = Fraction(1, ed.TWO_EIG_D) * np.array([[Fraction(int(v)) for v in row] for row in cc.k_inverse(b, identity)],
                                              dtype=object)
    vals = _fraction_vector(va)
    starts = rp[:-1].astype(np.int64)
    matvec = lambda v: np.add.reduceat(vals * v[ci], starts)
    precond = lambda r: (r.reshape(n0, b).dot(Ki.T)).ravel()          # K^-1 is symmetric; (I / d with K = I)
    dot = lambda u, v: sum(u * v, Fraction(0))
    rhs = _fraction_vector(s["rhs"])
    x = np.array([Fraction(0)] * n, dtype=object)
    r = rhs.copy()
    z = precond(r)
    assert np.array_equal(_fraction_vector(spmv.bsr_diag_apply_cpu(B, inv, s["rhs"])), z)      # the ordered fp32 sum is exact
    p = z.copy()
    rz = dot(r, z)
    worst = 0
    for step, (alpha_want, x_want) in enumerate(((2, s["x1"]), (2, s["x2"]))):
        assert _is_float32(p) and _is_float32(r) and _is_float32(z)
        worst = max(worst, _check_exact_scaled(rp, ci, va, p))
        q = matvec(p)
        assert _is_float32(q)
        alpha = rz / dot(p, q)
        assert alpha == alpha_want, (step, alpha)
        x = x + alpha * p
        r = r - alpha * q
        assert np.array_equal(x, _fraction_vector(x_want)), step
        z_float = spmv.bsr_diag_apply_cpu(B, inv, np.array([float(v) for v in r], np.float32))
        z = precond(r)
        assert np.array_equal(_fraction_vector(z_float), z), step
        rz_new = dot(r, z)
        if step == 0:
            assert rz_new / rz == Fraction(1, 2)
            rel1 = np.float32(np.sqrt(float(dot(r, r))) / np.sqrt(float(dot(rhs, rhs))))
            assert abs(int(rel1.view(np.int32)) - int(s["rel1"].view(np.int32))) <= 1
            p = z + Fraction(1, 2) * p
            rz = rz_new
    assert not r.any(), "r2 == 0"
    print("b", b, "n0", n0, "L", L, "identity", identity, "max row sum of |a||p| in units of p's last bit", worst)
    spmv.bsr_destroy(B)


# ---- BLOCK_JACOBI helps --------------------------------------------------------------------------------------
def test_block_jacobi_needs_fewer_steps_than_jacobi_in_the_restatement():
    n, b, rp, ci, va, rhs = cc.helps_system()
    x0 = np.zeros(n, np.float32)
    _, it_j, conv_j, _, _ = cc.restate(n, b, rp, ci, va, rhs, x0, 1e-6, 2000, cc.JACOBI)
    _, it_b, conv_b, _, _ = cc.restate(n, b, rp, ci, va, rhs, x0, 1e-6, 2000, cc.BLOCK_JACOBI)
    print("iterations to 1e-6: JACOBI", it_j, "BLOCK_JACOBI", it_b)
    assert conv_j and conv_b and it_b < it_j


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_the_float_cases_end_on_a_residual_the_reference_itself_is_sure_of(b):
    """cg_bsr_cases.float_cases: six realisations of the restatement (q = A p rounded from fp64 sums; summed in fp32;
    three with roundoff-sized noise on q; in the lane-group kernel's documented order, restated on the CPU) end after the same number of steps on relative residuals within 0.25 % of the
    first, a quarter of the 1 % the GPU test allows the device, and the restatement stops with its last residual at
    least 5 % below the tolerance and the one before at least 5 % above it (cg_bsr_cases.stop_margin).  Where either
    fails the final residual is no stable quantity of the iteration: a correct solve may stop a step apart from the
    reference, which the bound on the steps allows, and then cannot end on the reference's residual."""
    for n, base, seed in cc.float_cases(b):
        n, rp, ci, va, rhs = cc.float_system(n, b, base, seed)
        for precond in (cc.NONE, cc.JACOBI, cc.BLOCK_JACOBI):
            spread, steps = cc.reference_spread(n, b, rp, ci, va, rhs, 1e-5, precond)
            margin = cc.stop_margin(n, b, rp, ci, va, rhs, 1e-5, precond)
            print(b, n, base, seed, precond, "spread %.4f %%" % (100 * spread), "stop margin %.1f %%" % (100 * margin))
            assert spread <= 0.0025 and steps == 0, (b, n, base, seed, precond, spread, steps)
            assert margin >= cc.STOP_MARGIN, (b, n, base, seed, precond, margin)


# ---- argument rejections, nothing dereferenced ---------------------------------------------------------------
def test_solver_and_device_entry_checks_in_the_documented_order(spmv):
    cfg = lambda **kw: spmv.CGConfig(**kw)
    solve = lambda A, b=FAKE_B, x=FAKE_X, c=None: spmv.cg_solve_bsr(A, b, x, c)
    A = spmv.bsr_wrap_device(8, 8, 2, 5, FAKE_RP, FAKE_CI, FAKE_VA)
    R = spmv.bsr_wrap_device(8, 6, 2, 5, FAKE_RP, FAKE_CI, FAKE_VA)                   # not square
    Z = spmv.bsr_wrap_device(0, 0, 2, 0, FAKE_RP, None, None)                          # no rows
    NV = spmv.bsr_wrap_device(8, 8, 2, 5, FAKE_RP, FAKE_CI, None)                      # no values
    # null arguments first, then the shape, then "no rows", then the arrays
    assert solve(None).error_code == ARGUMENT
    assert solve(A, b=None).error_code == ARGUMENT and solve(A, x=None).error_code == ARGUMENT
    assert solve(R, b=None).error_code == ARGUMENT
    assert solve(R).error_code == DIMENSION
    assert solve(R, c=cfg(tolerance=-1.0)).error_code == DIMENSION
    res = solve(Z, c=cfg(tolerance=-1.0))                              # no rows: SUCCESS before the config is read
    assert (res.error_code, res.converged, res.iterations) == (OK, 1, 0)
    assert solve(NV).error_code == FORMAT
    assert solve(NV, c=cfg(tolerance=-1.0)).error_code == FORMAT
    # the config
    for bad in (cfg(tolerance=-1.0), cfg(tolerance=float("nan")), cfg(max_iterations=-1), cfg(preconditioner=3),
                cfg(preconditioner=-1), cfg(engine=1), cfg(engine=2), cfg(engine=-2)):
        assert solve(A, c=bad).error_code == ARGUMENT
        assert solve(A, b=FAKE_X, c=bad).error_code == ARGUMENT
    # overlapping ranges last: 8 floats each
    for precond in (cc.NONE, cc.JACOBI, cc.BLOCK_JACOBI):
        for engine in (-1, 0):
            c = cfg(preconditioner=precond, engine=engine)
            assert solve(A, b=FAKE_X, c=c).error_code == ARGUMENT
            assert solve(A, b=FAKE_X + 28, c=c).error_code == ARGUMENT
            assert solve(A, b=FAKE_X - 28, c=c).error_code == ARGUMENT
    # the device inverse and apply
    lib = spmv.lib()
    assert lib.spmv_c_bsr_diag_inverse_gpu(None, FAKE_X) == ARGUMENT and lib.spmv_c_bsr_diag_inverse_gpu(A, None) == ARGUMENT
    assert lib.spmv_c_bsr_diag_inverse_gpu(R, FAKE_X) == DIMENSION
    assert lib.spmv_c_bsr_diag_inverse_gpu(NV, FAKE_X) == FORMAT
    assert lib.spmv_c_bsr_diag_inverse_gpu(Z, FAKE_X) == OK
    for args in ((None, FAKE_VA, FAKE_B, FAKE_X), (A, None, FAKE_B, FAKE_X), (A, FAKE_VA, None, FAKE_X),
                 (A, FAKE_VA, FAKE_B, None)):
        assert lib.spmv_c_bsr_diag_apply(*args) == ARGUMENT
    assert lib.spmv_c_bsr_diag_apply(R, FAKE_VA, FAKE_B, FAKE_X) == DIMENSION
    assert lib.spmv_c_bsr_diag_apply(Z, FAKE_VA, FAKE_B, FAKE_X) == OK
    for M in (A, R, Z, NV):
        spmv.bsr_destroy(M)


def test_every_other_cg_entry_point_still_rejects_block_jacobi(spmv):
    A = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    c = spmv.CGConfig(preconditioner=cc.BLOCK_JACOBI, engine=0)
    assert spmv.cg_solve(A, FAKE_B, FAKE_X, c).error_code == ARGUMENT
    assert spmv.cg_solve(A, FAKE_B, FAKE_X, spmv.CGConfig(preconditioner=cc.BLOCK_JACOBI)).error_code == ARGUMENT
    results = spmv.cg_solve_multi(A, FAKE_B, FAKE_X, 2, config=c)
    assert [r.error_code for r in results] == [ARGUMENT, ARGUMENT]
    spmv.csr_destroy(A)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_the_host_routines_are_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-cg-bsr builds tests/cpp/bin/cg_bsr_host_sanitized (csrc/bsr_diag_host.cpp and the
    BSR host files it needs, with tests/cpp/cg_bsr_host_sanitized.cpp, under AddressSanitizer + UBSan); any sanitizer
    report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-cg-bsr"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "cg_bsr_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
