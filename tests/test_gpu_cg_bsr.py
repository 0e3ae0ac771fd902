"""cg_solve_bsr and the block-Jacobi routines (include/spmv/cg.h, include/spmv/bsr.h) on the device.

Zero tolerance unless said: bsr_diag_inverse_gpu and bsr_diag_apply against the host twins bit for bit (every block
size, ragged sizes, arrays as views at 4-, 8- and 12-byte offsets, guards around the outputs, past the inverse kernel's
grid cap); the exact two-step solves of tests/cg_bsr_cases.py at every block size x forced lane count x preconditioner,
and past every grid cap; float systems against the numpy restatement with test_gpu_cg.py's bounds; BLOCK_JACOBI needing
fewer steps than JACOBI; the behaviour rules of cg.h; and the C++ caller.

The one allowance in the exact tests is test_gpu_solver_trips.py's: relative_residual after ONE step is
float32(sqrt(r.r) / sqrt(b.b)) of exact fp64 sums, two square roots and a division the device may round differently
from numpy in the last place, so it may differ from the prediction by one float32 ulp.

The constants behind the sizes (csrc/device_common.h, csrc/cg_bsr.hip): kBlock = 256 threads; cg_bsr_update and
bsr_diag_inverse_kernel run on at most kVecBlocks = 1024 workgroups, so a trip of the update covers 1024 T rows with
T = kBlock - kBlock % b (255 for b = 3) and a trip of the inverse kernel 262 144 block rows; cg_bsr_spmv_dot and
cg_bsr_init run on at most kMaxResidentBlocks = 2048 workgroups of 256 / L block rows each."""
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import cg_bsr_cases as cc
import exact_data as ed
from conftest import ROOT

pytestmark = pytest.mark.gpu

NONE, JACOBI, BLOCK_JACOBI = cc.NONE, cc.JACOBI, cc.BLOCK_JACOBI
ARGUMENT = -8
TOL = 1e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, what=""):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


class Dev:
    """A BSR matrix on the device (bsr_from_arrays + bsr_to_gpu) with device b and x buffers."""

    def __init__(self, gpu, n, b, brp, bc, bv, rhs):
        self.gpu, self.n = gpu, n
        self.A = gpu.bsr_from_arrays(n, n, b, brp, bc, bv)
        assert gpu.bsr_to_gpu(self.A) == 0
        self.d_b, self.d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        self.d_b.copyFromHost(np.ascontiguousarray(rhs, np.float32), n)

    @classmethod
    def from_csr(cls, gpu, n, b, rp, ci, va, rhs):
        """through bsr_from_csr_cpu: ragged sizes get their padded last block from the library"""
        C = gpu.csr_from_arrays(n, n, rp, ci, va)
        H = gpu.bsr_create(0, 0, 2, 0)
        assert gpu.bsr_from_csr_cpu(H, C, b) == 0
        brp, bc, bv = gpu.bsr_host_arrays(H)
        gpu.csr_destroy(C)
        gpu.bsr_destroy(H)
        return cls(gpu, n, b, brp, bc, bv, rhs)

    def solve(self, x0=None, **cfg):
        x0 = np.zeros(self.n, np.float32) if x0 is None else np.asarray(x0, np.float32)
        self.d_x.copyFromHost(x0, self.n)
        res = self.gpu.cg_solve_bsr(self.A, self.d_b, self.d_x, self.gpu.CGConfig(**cfg))
        return res, self.d_x.copyToHost(self.n)

    def close(self):
        self.gpu.bsr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def lifted(gpu, n0, L, b, identity):
    s = cc.lifted_system(n0, L, b, identity)
    return s, Dev(gpu, s["n"], b, s["brp"], s["bc"], s["bv"], s["rhs"])


def assert_two_steps(dev, s, precond, what):
    """The full solve and the solve stopped after one step (module docstring)."""
    res, x = dev.solve(tolerance=TOL, max_iterations=50, preconditioner=precond, engine=0)
    what = what + (precond, res.iterations, res.relative_residual)
    assert res.error_code == 0, dev.gpu.spmv_error_string(res.error_code)
    assert res.iterations == 2 and res.converged == 1 and res.breakdown == 0, what
    assert res.relative_residual == 0.0, what
    assert_bits(x, s["x2"], what)
    res, x = dev.solve(tolerance=0.0, max_iterations=1, preconditioner=precond, engine=0)
    got, want = np.float32(res.relative_residual), s["rel1"]
    ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
    print("one step", what, "relative_residual", got, "predicted", want, "ulps", ulps)
    assert res.error_code == 0 and res.iterations == 1 and res.converged == 0 and res.breakdown == 0, what
    assert_bits(x, s["x1"], what)
    assert ulps <= 1, (what, got, want)


def both_lifts(gpu, n0, L, b, what):
    """NONE and JACOBI on the K = I lift, BLOCK_JACOBI on the K lift"""
    s, dev = lifted(gpu, n0, L, b, True)
    try:
        assert_two_steps(dev, s, NONE, what)
        assert_two_steps(dev, s, JACOBI, what)
    finally:
        dev.close()
    s, dev = lifted(gpu, n0, L, b, False)
    try:
        assert_two_steps(dev, s, BLOCK_JACOBI, what)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 1. inverse and apply
def _float_case(n, b, seed):
    n, rp, ci, va = cc.block_spd(n, b, seed=seed)
    r = np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)
    return n, rp, ci, va, r


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_inverse_and_apply_equal_the_host_twins_as_views(gpu, b):
    """1, b-1, b, b+1 rows, ragged sizes of a few hundred rows and 4097 block rows; the value array, the inverses, r and
    z as views at 4-, 8- and 12-byte offsets inside larger buffers, with the padding around the outputs never written."""
    sizes = sorted({1, max(b - 1, 1), b, b + 1, 37 * b + 1, 50 * b - 1, 4097 * b - (b - 1)})
    for k, n in enumerate(sizes):
        offset = 1 + k % 3
        n, rp, ci, va, r = _float_case(n, b, seed=100 + b)
        C = gpu.csr_from_arrays(n, n, rp, ci, va)
        H = gpu.bsr_create(0, 0, 2, 0)
        assert gpu.bsr_from_csr_cpu(H, C, b) == 0
        brp, bc, bv = gpu.bsr_host_arrays(H)
        status, inv_want = gpu.bsr_diag_inverse_cpu(H)
        assert status == 0, (b, n)
        z_want = gpu.bsr_diag_apply_cpu(H, inv_want, r)
        with av.Views(gpu) as views:
            v_rp = views.view(brp, 0, np.int32(bc.size))
            v_bc = views.view(bc, 3 - k % 3, np.int32(0))
            v_bv = views.view(bv, offset, np.float32(ed.VIEW_POISON))
            W = gpu.bsr_wrap_device(n, n, b, int(bc.size), v_rp.ptr, v_bc.ptr, v_bv.ptr)
            v_inv = views.out(inv_want.size, offset)
            v_r = views.x(r, (offset + 1) % 4)
            v_z = views.out(n, (offset + 2) % 4)
            try:
                assert gpu.bsr_diag_inverse_gpu(W, v_inv.ptr) == 0, (b, n)
                assert_bits(v_inv.download(), inv_want, ("inverse", b, n, offset))
                assert gpu.bsr_diag_apply(W, v_inv.ptr, v_r.ptr, v_z.ptr) == 0
                assert_bits(v_z.download(), z_want, ("apply", b, n, offset))
                views.check_guards((b, n))
            finally:
                gpu.bsr_destroy(W)
        gpu.bsr_destroy(H)
        gpu.csr_destroy(C)


def test_inverse_past_its_grid_cap(gpu):
    """262 144 + 257 block rows of b = 2 (a block-diagonal matrix): bsr_diag_inverse_kernel's second trip, and
    bsr_diag_apply_kernel's third."""
    b, nb = 2, cc.VEC_BLOCKS * cc.K_BLOCK + 257
    n = nb * b - 1
    rng = np.random.default_rng(7)
    Q = rng.uniform(-1.0, 1.0, size=(nb, b, b))
    blocks = (np.einsum("eki,ekj->eij", Q, Q) + 0.1 * np.eye(b)[None]).astype(np.float32)
    blocks[-1, 1, :] = blocks[-1, :, 1] = 0.0                          # the padding of the ragged last block
    brp, bc = np.arange(nb + 1, dtype=np.int32), np.arange(nb, dtype=np.int32)
    r = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    dev = Dev(gpu, n, b, brp, bc, blocks.ravel(), r)
    d_inv, d_z = gpu.CudaBuffer(nb * b * b), gpu.CudaBuffer(n)
    try:
        status, want = gpu.bsr_diag_inverse_cpu(dev.A)
        assert status == 0 and gpu.bsr_diag_inverse_gpu(dev.A, d_inv) == 0
        assert_bits(d_inv.copyToHost(nb * b * b), want)
        assert gpu.bsr_diag_apply(dev.A, d_inv, dev.d_b, d_z) == 0
        assert_bits(d_z.copyToHost(n), gpu.bsr_diag_apply_cpu(dev.A, want, r))
    finally:
        dev.close()
        d_inv.release()
        d_z.release()


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_device_side_rejections_leave_x_untouched(gpu, b):
    """A block row without a diagonal block, a zero, negative, NaN and Inf pivot: bsr_diag_inverse_gpu and cg_solve_bsr
    with BLOCK_JACOBI say INVALID_ARGUMENT; JACOBI rejects a (k,k) entry that is not > 0; NONE solves regardless; d_x is
    not written by a rejected solve."""
    n = 40 * b - 1
    n, rp, ci, va, rhs = _float_case(n, b, seed=300 + b)
    rows = np.repeat(np.arange(n), np.diff(rp))
    x0 = np.linspace(-1.0, 1.0, n).astype(np.float32)
    target = 7 * b + (b - 1)                                           # the last row of block row 7
    on_pivot = np.flatnonzero((rows == target) & (ci == target))[0]
    cases = {"zero": 0.0, "negative": -1.0, "nan": np.nan, "inf": np.inf, "missing": None}
    for name, value in cases.items():
        va2, ci2, rp2 = va.copy(), ci, rp
        if value is None:                                              # block row 7 loses its diagonal block
            drop = (rows // b == 7) & (ci // b == 7)
            va2, ci2 = va[~drop], ci[~drop]
            rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[~drop], minlength=n))]).astype(np.int32)
        else:
            va2[on_pivot] = value
        dev = Dev.from_csr(gpu, n, b, rp2, ci2, va2, rhs)
        d_inv = gpu.CudaBuffer(dev.A.contents.num_block_rows * b * b)
        try:
            assert gpu.bsr_diag_inverse_gpu(dev.A, d_inv) == ARGUMENT, (b, name)
            assert gpu.bsr_diag_inverse_cpu(dev.A)[0] == ARGUMENT, (b, name)
            res, x = dev.solve(x0=x0, preconditioner=BLOCK_JACOBI)
            assert res.error_code == ARGUMENT, (b, name, res.error_code)
            assert_bits(x, x0, (b, name))
            res, x = dev.solve(x0=x0, preconditioner=JACOBI)
            jacobi_bad = name in ("zero", "negative", "nan", "missing")          # +Inf is > 0: cg_solve's rule
            assert (res.error_code == ARGUMENT) == jacobi_bad, (b, name, res.error_code)
            if jacobi_bad:
                assert_bits(x, x0, (b, name))
            res, _ = dev.solve(x0=x0, preconditioner=NONE, max_iterations=3)
            assert res.error_code == 0, (b, name)
        finally:
            dev.close()
            d_inv.release()


# ------------------------------------------------------------------------------------------ 2. exact two-step solves
@pytest.mark.parametrize("n0", [257, 1201])
@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_exact_two_step_solves_at_every_lane_count(gpu, monkeypatch, b, n0):
    """b x forced bsr_lanes in 1 .. 64 x (NONE, JACOBI on the K = I lift; BLOCK_JACOBI on the K lift): iterations == 2,
    converged, relative_residual == 0, x == x2 to the bit; stopped after one step x == x1."""
    devs = [lifted(gpu, n0, 1, b, True), lifted(gpu, n0, 1, b, False)]
    try:
        for lanes in cc.LANES:
            cc.forced(monkeypatch, lanes)
            assert_two_steps(devs[0][1], devs[0][0], NONE, (b, n0, lanes))
            assert_two_steps(devs[0][1], devs[0][0], JACOBI, (b, n0, lanes))
            assert_two_steps(devs[1][1], devs[1][0], BLOCK_JACOBI, (b, n0, lanes))
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        assert_two_steps(devs[1][1], devs[1][0], BLOCK_JACOBI, (b, n0, "natural lanes"))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        for _, dev in devs:
            dev.close()


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_exact_two_step_solves_on_a_value_array_that_is_a_view(gpu, monkeypatch, b):
    """The values 4, 8 and 12 bytes past a 16-byte boundary: cg_bsr_spmv_dot<B, LANES, false> and cg_bsr_init<.., false>,
    the dword form of the block load, for the block sizes that otherwise take 16-byte loads."""
    s = cc.lifted_system(257, 1, b, False)
    n = s["n"]
    d_b, d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_b.copyFromHost(s["rhs"], n)
    try:
        for offset in (1, 2, 3):
            for lanes in (1, 4, 64):
                cc.forced(monkeypatch, lanes)
                with av.Views(gpu) as views:
                    v_rp = views.view(s["brp"], 0, np.int32(s["bc"].size))
                    v_bc = views.view(s["bc"], offset, np.int32(0))
                    v_bv = views.view(s["bv"], offset, np.float32(ed.VIEW_POISON))
                    W = gpu.bsr_wrap_device(n, n, b, int(s["bc"].size), v_rp.ptr, v_bc.ptr, v_bv.ptr)
                    try:
                        d_x.copyFromHost(np.zeros(n, np.float32), n)
                        res = gpu.cg_solve_bsr(W, d_b, d_x, gpu.CGConfig(tolerance=TOL, preconditioner=BLOCK_JACOBI))
                        what = (b, offset, lanes, res.iterations, res.relative_residual)
                        assert (res.error_code, res.iterations, res.converged, res.relative_residual) == (0, 2, 1, 0.0), what
                        assert_bits(d_x.copyToHost(n), s["x2"], what)
                    finally:
                        gpu.bsr_destroy(W)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        d_b.release()
        d_x.release()


# ------------------------------------------------------------------------------------------ 3. past the caps
def _cap_cases():
    cases = []
    for b in cc.BLOCK_DIMS:
        u = cc.update_trip(b) // b                                     # block rows of one trip of cg_bsr_update
        assert u * b == cc.update_trip(b)
        for n0 in (u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1):      # below / at / above one trip, and two trips
            cases.append((b, n0, None))
        for lanes in (64, 1):                                          # one trip of the block-row kernels
            r = cc.row_trip(lanes)
            for n0 in (r - 1, r, r + 1):
                cases.append((b, n0, lanes))
    return cases


CAP_CASES = _cap_cases()


@pytest.mark.parametrize("b,n0,lanes", CAP_CASES, ids=["b%d_n%d_L%s" % c for c in CAP_CASES])
def test_exact_two_step_solves_past_the_grid_caps(gpu, monkeypatch, b, n0, lanes):
    """N = b n0 just below, at and just above one trip of cg_bsr_update (1024 T rows; b = 3: T = 255, 261 120 rows, no
    power of two), the same around two trips (at 2 u every workgroup makes exactly two trips and the LDS line swaps
    once with no third trip; at 2 u - 1 the second trip's last block row is missing), and around one trip of cg_bsr_spmv_dot / cg_bsr_init at 64 lanes (8192 block rows)
    and at one lane (524 288 block rows).  At one lane both grids sit at their caps and the solve's partial-sum array
    is 4 * 2048 + 2 * 1024 = 10 240 doubles, a whole number of 4 KiB pages: the size at which cg_start_kernel once
    read the double past the end (the note in test_gpu_solver_trips.test_cg_every_trip)."""
    if lanes is not None:
        cc.forced(monkeypatch, lanes)
    try:
        both_lifts(gpu, n0, 1, b, (b, n0, lanes))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


# ------------------------------------------------------------------------------------------ 4. float systems
@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_restatement_parity_on_float_systems(gpu, b):
    """test_gpu_cg.py's bounds: |iterations - ref| <= 2, relative_residual within 1 % of the reference's, true residual
    <= max(4 tol, 2 x the reference's), for all three preconditioners on the systems of cg_bsr_cases.float_cases (ragged
    sizes of a few thousand rows, on which the reference itself is stable to a quarter of the 1 %).
    The systems are pre-screened on the CPU (cg_bsr_cases.float_cases says how, tests/test_cg_bsr_host.py asserts it).
    A failure of the 1 % bound on a NEW seed or size is therefore not by itself a kernel bug: first run the host test on
    it; the residual a solve ends on is no stable quantity on a system that misses the screening.  The comparison that
    needs no screening is test_fixed_step_runs_match_the_restatement below."""
    for n, base, seed in cc.float_cases(b):
        n, rp, ci, va, rhs = cc.float_system(n, b, base, seed)
        dev = Dev.from_csr(gpu, n, b, rp, ci, va, rhs)
        try:
            for precond in (NONE, JACOBI, BLOCK_JACOBI):
                tol = 1e-5
                res, x = dev.solve(tolerance=tol, preconditioner=precond, engine=0, max_iterations=5000)
                assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
                x_ref, it_ref, conv_ref, brk_ref, rel_ref = cc.restate(n, b, rp, ci, va, rhs, np.zeros(n), tol, 5000,
                                                                       precond)
                what = (b, n, precond, res.iterations, it_ref)
                print(what, res.relative_residual, rel_ref)
                assert abs(res.iterations - it_ref) <= 2, what
                assert bool(res.converged) == conv_ref and not res.breakdown and not brk_ref, what
                assert abs(res.relative_residual - rel_ref) <= 0.01 * rel_ref, (what, res.relative_residual, rel_ref)
                assert res.relative_residual <= tol
                bound = max(4 * tol, 2 * cc.true_residual(rp, ci, va, rhs, x_ref))
                assert cc.true_residual(rp, ci, va, rhs, x) <= bound, what
                assert res.elapsed_ms > 0
        finally:
            dev.close()


@pytest.mark.parametrize("b", cc.BLOCK_DIMS)
def test_fixed_step_runs_match_the_restatement(gpu, b):
    n = cc.ragged_sizes(b)[0]
    n, rp, ci, va = cc.block_spd(n, b, seed=40 + b)
    rhs = np.random.default_rng(n + 1).uniform(-1.0, 1.0, n).astype(np.float32)
    dev = Dev.from_csr(gpu, n, b, rp, ci, va, rhs)
    try:
        for precond in (NONE, JACOBI, BLOCK_JACOBI):
            for k in (1, 2, 5):
                res, x = dev.solve(tolerance=1e-7, max_iterations=k, preconditioner=precond, engine=0)
                assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
                x_ref, it_ref, conv_ref, _, _ = cc.restate(n, b, rp, ci, va, rhs, np.zeros(n), 1e-7, k, precond)
                assert it_ref == k and not conv_ref
                err = np.linalg.norm(x.astype(np.float64) - x_ref) / np.linalg.norm(x_ref.astype(np.float64))
                assert err <= 1e-5, (b, precond, k, err)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 5. BLOCK_JACOBI helps
def test_block_jacobi_needs_fewer_steps_than_jacobi(gpu):
    n, b, rp, ci, va, rhs = cc.helps_system()
    dev = Dev.from_csr(gpu, n, b, rp, ci, va, rhs)
    try:
        res_j, _ = dev.solve(tolerance=1e-6, preconditioner=JACOBI, max_iterations=2000)
        res_b, _ = dev.solve(tolerance=1e-6, preconditioner=BLOCK_JACOBI, max_iterations=2000)
        print("iterations to 1e-6: JACOBI", res_j.iterations, "BLOCK_JACOBI", res_b.iterations)
        assert res_j.error_code == 0 and res_b.error_code == 0 and res_j.converged and res_b.converged
        assert res_b.iterations < res_j.iterations
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. behaviour rules
def _behaviour_system(gpu, b=3):
    n = cc.ragged_sizes(b)[0]
    n, rp, ci, va = cc.block_spd(n, b, seed=60 + b)
    rhs = np.random.default_rng(3).uniform(-1.0, 1.0, n).astype(np.float32)
    return n, rp, ci, va, rhs, Dev.from_csr(gpu, n, b, rp, ci, va, rhs)


def test_runs_repeat_bit_for_bit_also_on_a_side_stream(gpu):
    import torch
    n, rp, ci, va, rhs, dev = _behaviour_system(gpu)
    side = torch.cuda.Stream()
    try:
        for precond in (NONE, JACOBI, BLOCK_JACOBI):
            first, x_first = dev.solve(tolerance=1e-6, preconditioner=precond)
            again, x_again = dev.solve(tolerance=1e-6, preconditioner=precond)
            assert first.error_code == 0 and first.converged
            assert (first.iterations, first.relative_residual) == (again.iterations, again.relative_residual)
            assert_bits(x_again, x_first, precond)
            gpu.set_stream(side.cuda_stream)
            other, x_other = dev.solve(tolerance=1e-6, preconditioner=precond)
            gpu.set_stream(None)
            assert (other.error_code, other.iterations, other.relative_residual) == (0, first.iterations,
                                                                                     first.relative_residual)
            assert_bits(x_other, x_first, (precond, "side stream"))
    finally:
        gpu.set_stream(None)
        dev.close()


def test_a_solve_stopped_at_the_reported_count_equals_the_full_solve(gpu):
    """... and one step more moves nothing: the loop kernels honour `done`."""
    n, rp, ci, va, rhs, dev = _behaviour_system(gpu, b=4)
    try:
        for precond in (NONE, JACOBI, BLOCK_JACOBI):
            full, x_full = dev.solve(tolerance=1e-5, preconditioner=precond, max_iterations=5000)
            assert full.error_code == 0 and full.converged and full.iterations > 2
            for extra in (0, 1):
                res, x = dev.solve(tolerance=1e-5, preconditioner=precond, max_iterations=full.iterations + extra)
                assert (res.iterations, res.converged, res.relative_residual) == (full.iterations, 1,
                                                                                   full.relative_residual)
                assert_bits(x, x_full, (precond, extra))
    finally:
        dev.close()


def test_zero_steps_zero_b_and_a_converged_guess(gpu):
    n, rp, ci, va, rhs, dev = _behaviour_system(gpu, b=2)
    try:
        x0 = np.full(n, 0.5, np.float32)
        for precond in (NONE, JACOBI, BLOCK_JACOBI):
            res, x = dev.solve(x0=x0, max_iterations=0, preconditioner=precond)           # max_iterations = 0
            assert (res.error_code, res.iterations, res.converged) == (0, 0, 0)
            assert_bits(x, x0)
            solved, x_solved = dev.solve(tolerance=1e-5, preconditioner=precond)          # a converged initial guess
            assert solved.converged and solved.iterations > 0
            res, x = dev.solve(x0=x_solved, tolerance=1e-3, preconditioner=precond)
            assert (res.error_code, res.converged, res.iterations) == (0, 1, 0) and res.relative_residual <= 1e-3
            assert_bits(x, x_solved)
        dev.d_b.copyFromHost(np.zeros(n, np.float32), n)                                   # b = 0
        for precond in (NONE, JACOBI, BLOCK_JACOBI):
            res, x = dev.solve(x0=np.full(n, 3.0, np.float32), preconditioner=precond)
            assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
            assert_bits(x, np.zeros(n, np.float32))
    finally:
        dev.close()


def test_an_indefinite_matrix_breaks_down_at_the_last_good_iterate(gpu):
    """diag(1, 1, -1, -1) in 2 x 2 blocks with b = (1, 1, 1, 1): p.Ap = 0 at the first step, x stays x0; with
    BLOCK_JACOBI the negative block is rejected as a bad pivot instead."""
    brp, bc = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    bv = np.array([1, 0, 0, 1, -1, 0, 0, -1], np.float32)
    dev = Dev(gpu, 4, 2, brp, bc, bv, np.ones(4, np.float32))
    try:
        x0 = np.array([0.5, -0.25, 2.0, 1.0], np.float32)
        res, x = dev.solve(x0=np.zeros(4, np.float32), preconditioner=NONE)
        assert res.error_code == 0 and res.breakdown == 1 and not res.converged and res.iterations == 0
        assert_bits(x, np.zeros(4, np.float32))
        res, x = dev.solve(x0=x0, preconditioner=BLOCK_JACOBI)
        assert res.error_code == ARGUMENT
        assert_bits(x, x0)
    finally:
        dev.close()


def test_a_late_breakdown_keeps_the_iterate_of_the_last_committed_step(gpu):
    """diag(1, 2, 3, 4, 5, -1/4) in 2 x 2 blocks with a small right-hand side in the negative direction: the first steps
    are good ones (p.Ap > 0) and commit; once the positive part is resolved p.Ap turns negative.  The restatement
    commits 4 steps and breaks down in the 5th.  The solve reports breakdown with the count of the committed steps, and
    x is bit for bit the x of a solve stopped at that count: cg_bsr_update wrote nothing in the step that broke down."""
    d = np.array([1, 2, 3, 4, 5, -0.25], np.float32)
    rhs = np.array([1, 1, 1, 1, 1, 0.125], np.float32)
    n = 6
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    _, it_ref, conv_ref, brk_ref, rel_ref = cc.restate(n, 2, rp, ci, d, rhs, np.zeros(n), 1e-6, 50, NONE)
    assert (it_ref, conv_ref, brk_ref) == (4, False, True)
    dev = Dev.from_csr(gpu, n, 2, rp, ci, d, rhs)
    try:
        res, x = dev.solve(tolerance=1e-6, max_iterations=50, preconditioner=NONE)
        what = (res.iterations, res.relative_residual, rel_ref)
        assert res.error_code == 0 and res.breakdown == 1 and not res.converged, what
        assert res.iterations == it_ref, what
        assert abs(res.relative_residual - rel_ref) <= 1e-5 * rel_ref, what
        stopped, x_stopped = dev.solve(tolerance=1e-6, max_iterations=res.iterations, preconditioner=NONE)
        assert (stopped.iterations, stopped.breakdown, stopped.converged) == (res.iterations, 0, 0)
        assert stopped.relative_residual == res.relative_residual
        assert_bits(x, x_stopped, what)
        assert np.all(np.isfinite(x))
    finally:
        dev.close()


def test_engine_one_is_rejected(gpu):
    n, rp, ci, va, rhs, dev = _behaviour_system(gpu, b=2)
    try:
        x0 = np.full(n, 0.25, np.float32)
        res, x = dev.solve(x0=x0, engine=1)
        assert res.error_code == ARGUMENT
        assert_bits(x, x0)
        assert dev.solve(engine=-1, tolerance=1e-5)[0].converged and dev.solve(engine=0, tolerance=1e-5)[0].converged
    finally:
        dev.close()


@pytest.mark.parametrize("b", [3, 4])
def test_a_converted_matrix_solves_and_a_refill_is_not_stale(gpu, b):
    """bsr_from_csr_gpu's output goes straight into cg_solve_bsr; after bsr_from_csr_numeric with new values the next
    solve equals a solve on a matrix built from those values: nothing stale is cached."""
    n = cc.ragged_sizes(b)[0]
    n, rp, ci, va = cc.block_spd(n, b, seed=80 + b)
    rhs = np.random.default_rng(9).uniform(-1.0, 1.0, n).astype(np.float32)
    va2 = (va * np.float32(1.5)).astype(np.float32)
    on = np.repeat(np.arange(n), np.diff(rp)) == ci
    va2[on] *= np.float32(2.0)                                         # another matrix, still SPD: another iteration
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    B = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_gpu(B, A, b).error_code == 0
    d_b, d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_b.copyFromHost(rhs, n)
    fresh1 = Dev.from_csr(gpu, n, b, rp, ci, va, rhs)
    fresh2 = Dev.from_csr(gpu, n, b, rp, ci, va2, rhs)
    try:
        def solve(precond):
            d_x.copyFromHost(np.zeros(n, np.float32), n)
            res = gpu.cg_solve_bsr(B, d_b, d_x, gpu.CGConfig(tolerance=1e-6, preconditioner=precond))
            assert res.error_code == 0 and res.converged
            return res, d_x.copyToHost(n)
        for precond in (JACOBI, BLOCK_JACOBI):
            res, x = solve(precond)
            want, x_want = fresh1.solve(tolerance=1e-6, preconditioner=precond)
            assert (res.iterations, res.relative_residual) == (want.iterations, want.relative_residual)
            assert_bits(x, x_want, ("converted", precond))
        A2 = gpu.csr_from_arrays(n, n, rp, ci, va2)
        assert gpu.csr_to_gpu(A2) == 0 and gpu.bsr_from_csr_numeric(B, A2).error_code == 0
        gpu.csr_destroy(A2)
        for precond in (JACOBI, BLOCK_JACOBI):
            res, x = solve(precond)
            want, x_want = fresh2.solve(tolerance=1e-6, preconditioner=precond)
            old, x_old = fresh1.solve(tolerance=1e-6, preconditioner=precond)
            assert (res.iterations, res.relative_residual) == (want.iterations, want.relative_residual)
            assert_bits(x, x_want, ("refilled", precond))
            assert not np.array_equal(bits(x), bits(x_old))
    finally:
        fresh1.close()
        fresh2.close()
        gpu.bsr_destroy(B)
        gpu.csr_destroy(A)
        d_b.release()
        d_x.release()


# ------------------------------------------------------------------------------------------ 7. the C++ caller
def test_cpp_cg_bsr_smoke(gpu):
    """tests/cpp/cg_bsr_smoke.cpp through spmv/cg.h, spmv/bsr.h and CudaBuffer, compiled by __graft_entry__.build()."""
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "cg_bsr_smoke")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
