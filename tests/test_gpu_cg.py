"""cg_solve (include/spmv/cg.h) on the device.

The solver is checked against a numpy restatement that follows the documented numerics (fp32 vectors, fp64 dot
products of the fp32 entries, alpha and beta rounded to fp32 and applied as multiply-adds, z = r * dinv, the stop
test sqrt(r.r) <= tol * ||b|| after every step), against known answers, for its argument rejections on the device,
for run-to-run reproducibility, for agreement between its engines, and through a C++ caller."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
NONE, JACOBI = 0, 1
TILED_SMALL = "min_cols=1,min_nnz=1"


# ------------------------------------------------------------------------------------------ helpers
def diag_of(n, rp, ci, va):
    """(fp32 sum of the stored (i,i) entries in storage order, whether a row has one)"""
    d = np.zeros(n, np.float32)
    found = np.zeros(n, bool)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    on = np.flatnonzero(ci == rows)
    for j in on:                                  # test matrices hold one diagonal entry per row
        d[rows[j]] = np.float32(d[rows[j]] + va[j])
        found[rows[j]] = True
    return d, found


def spmv32(rp, ci, va, x):
    return spd.spmv64(rp, ci, va, x).astype(np.float32)


def restate(n, rp, ci, va, b, x0, tol, max_iter=1000, precond=JACOBI):
    """numpy PCG under cg.h's numeric rules; returns (x, iterations, converged, breakdown, relative residual)"""
    b = np.asarray(b, np.float32)
    x = np.asarray(x0, np.float32).copy()
    if precond == JACOBI:
        d, _ = diag_of(n, rp, ci, va)
        dinv = (np.float32(1.0) / d).astype(np.float32)
    else:
        dinv = np.ones(n, np.float32)
    dot = lambda a, c: float(np.dot(a.astype(np.float64), c.astype(np.float64)))
    r = (b - spmv32(rp, ci, va, x)).astype(np.float32)
    z = (r * dinv).astype(np.float32)
    p = z.copy()
    rz, rr, bb = dot(r, z), dot(r, r), dot(b, b)
    if bb == 0.0:
        return np.zeros(n, np.float32), 0, True, False, 0.0
    bnorm = np.sqrt(bb)
    thr = float(np.float32(tol)) * bnorm
    if np.sqrt(rr) <= thr:
        return x, 0, True, False, np.sqrt(rr) / bnorm
    if not rz > 0:
        return x, 0, False, True, np.sqrt(rr) / bnorm
    it, conv, brk, rel = 0, False, False, np.sqrt(rr) / bnorm
    for k in range(max_iter):
        q = spmv32(rp, ci, va, p)
        pq = dot(p, q)
        if not pq > 0:
            brk = True
            break
        a = np.float64(np.float32(rz / pq))
        x = (a * p.astype(np.float64) + x).astype(np.float32)
        r = (-a * q.astype(np.float64) + r).astype(np.float32)
        z = (r * dinv).astype(np.float32)
        rz_new, rr = dot(r, z), dot(r, r)
        it, rel = k + 1, np.sqrt(rr) / bnorm
        if np.sqrt(rr) <= thr:
            conv = True
            break
        if not rz_new > 0:
            brk = True
            break
        beta = np.float64(np.float32(rz_new / rz))
        p = (beta * p.astype(np.float64) + z).astype(np.float32)
        rz = rz_new
    return x, it, conv, brk, rel


def true_residual(rp, ci, va, b, x):
    b64 = np.asarray(b, np.float64)
    return float(np.linalg.norm(b64 - spd.spmv64(rp, ci, va, x)) / np.linalg.norm(b64))


class System:
    """A matrix on the device (csr_from_arrays + csr_to_gpu) with device b and x buffers."""

    def __init__(self, gpu, n, rp, ci, va, seed=1):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        rng = np.random.default_rng(seed)
        self.b = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        self.d_b = gpu.CudaBuffer(n)
        self.d_x = gpu.CudaBuffer(n)
        self.d_b.copyFromHost(self.b, n)

    def solve(self, x0=None, **cfg):
        x0 = np.zeros(self.n, np.float32) if x0 is None else np.asarray(x0, np.float32)
        self.d_x.copyFromHost(x0, self.n)
        res = self.gpu.cg_solve(self.A, self.d_b, self.d_x, self.gpu.CGConfig(**cfg))
        return res, self.d_x.copyToHost(self.n)

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def small_dense_system(gpu, dense, b):
    dense = np.asarray(dense, np.float32)
    n = dense.shape[0]
    A = gpu.csr_create(0, 0, 0)
    assert gpu.csr_from_dense(A, dense, n, n) == 0 and gpu.csr_to_gpu(A) == 0
    d_b, d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_b.copyFromHost(np.asarray(b, np.float32), n)
    return A, d_b, d_x


MATRICES = {
    "poisson2d_64": lambda: spd.poisson2d(64),
    "poisson2d_256": lambda: spd.poisson2d(256),
    "random_spd_1e5": lambda: spd.random_spd(100_000, 7, seed=3),
}


# ------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", list(MATRICES))
def test_restatement_parity(gpu, name):
    n, rp, ci, va = MATRICES[name]()
    s = System(gpu, n, rp, ci, va)
    try:
        for precond in (NONE, JACOBI):
            for tol in (1e-4, 1e-5):
                res, x = s.solve(tolerance=tol, preconditioner=precond, engine=0, max_iterations=5000)
                assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
                x_ref, it_ref, conv_ref, brk_ref, rel_ref = restate(n, rp, ci, va, s.b, np.zeros(n), tol, 5000,
                                                                    precond)
                what = (name, precond, tol, res.iterations, it_ref)
                assert abs(res.iterations - it_ref) <= 2, what
                assert bool(res.converged) == conv_ref and not res.breakdown and not brk_ref, what
                assert abs(res.relative_residual - rel_ref) <= 0.01 * rel_ref, (what, res.relative_residual, rel_ref)
                assert res.relative_residual <= tol
                bound = max(4 * tol, 2 * true_residual(rp, ci, va, s.b, x_ref))
                assert true_residual(rp, ci, va, s.b, x) <= bound, what
                assert res.elapsed_ms > 0
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ known answers
def test_positive_diagonal_matrix_converges_in_one_jacobi_step(gpu):
    n = 1000
    rng = np.random.default_rng(5)
    d = np.ldexp(np.float32(1.0), rng.integers(-3, 6, n)).astype(np.float32)     # powers of two: b/d is exact
    rp = np.arange(n + 1, dtype=np.int32)
    ci = np.arange(n, dtype=np.int32)
    s = System(gpu, n, rp, ci, d)
    try:
        res, x = s.solve(tolerance=1e-6, preconditioner=JACOBI, engine=0)
        assert res.error_code == 0 and res.converged and res.iterations == 1 and not res.breakdown
        want = (s.b / d).astype(np.float32)
        ulps = np.abs(x.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1
    finally:
        s.close()


def test_zero_b_writes_zeros(gpu):
    n, rp, ci, va = spd.poisson2d(16)
    s = System(gpu, n, rp, ci, va)
    try:
        s.d_b.copyFromHost(np.zeros(n, np.float32), n)
        res, x = s.solve(x0=np.full(n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(n, np.float32))
    finally:
        s.close()


def test_good_initial_guess_returns_at_once_and_leaves_x_alone(gpu):
    n, rp, ci, va = spd.poisson2d(32)
    s = System(gpu, n, rp, ci, va)
    try:
        res, x_solved = s.solve(tolerance=1e-5)
        assert res.converged and res.iterations > 0
        res2, x2 = s.solve(x0=x_solved, tolerance=1e-3)
        assert (res2.error_code, res2.converged, res2.iterations) == (0, 1, 0)
        assert np.array_equal(x2.view(np.uint32), x_solved.view(np.uint32))
        assert res2.relative_residual <= 1e-3
    finally:
        s.close()


def test_max_iterations_stops_there_and_matches_the_restatement(gpu):
    n, rp, ci, va = spd.poisson2d(64)
    s = System(gpu, n, rp, ci, va)
    try:
        for precond in (NONE, JACOBI):
            for k in (1, 5, 20):
                res, x = s.solve(tolerance=1e-7, max_iterations=k, preconditioner=precond, engine=0)
                assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
                x_ref, it_ref, conv_ref, _, _ = restate(n, rp, ci, va, s.b, np.zeros(n), 1e-7, k, precond)
                assert it_ref == k and not conv_ref
                err = np.linalg.norm(x.astype(np.float64) - x_ref) / np.linalg.norm(x_ref.astype(np.float64))
                assert err <= 1e-5, (precond, k, err)
        res, x = s.solve(max_iterations=0, x0=np.full(n, 0.5, np.float32))
        assert (res.error_code, res.iterations, res.converged) == (0, 0, 0)
        assert np.all(x == np.float32(0.5))
    finally:
        s.close()


def test_indefinite_matrix_breaks_down_with_finite_x(gpu):
    A, d_b, d_x = small_dense_system(gpu, [[1.0, 0.0], [0.0, -1.0]], [1.0, 1.0])
    try:
        d_x.copyFromHost(np.zeros(2, np.float32), 2)
        res = gpu.cg_solve(A, d_b, d_x, gpu.CGConfig(preconditioner=NONE))
        x = d_x.copyToHost(2)
        assert res.error_code == 0 and res.breakdown == 1 and not res.converged
        assert np.all(np.isfinite(x)) and np.isfinite(res.relative_residual)
    finally:
        gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------------ JACOBI rejections
@pytest.mark.parametrize("case", ["zero", "negative", "missing"])
def test_jacobi_rejects_a_bad_diagonal_and_leaves_x_untouched(gpu, case):
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, 3, 0, 1, 1, 5]
    elif case == "negative":                    # (2,2) = -2
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [4, .5, .5, 3, -2, 5]
    else:                                       # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [4, .5, .5, 3, 1, 1]
    A = gpu.csr_from_arrays(4, 4, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    d_b, d_x = gpu.CudaBuffer(4), gpu.CudaBuffer(4)
    d_b.copyFromHost(np.ones(4, np.float32), 4)
    x0 = np.array([7.0, -1.0, 2.5, 0.25], np.float32)
    d_x.copyFromHost(x0, 4)
    try:
        res = gpu.cg_solve(A, d_b, d_x, gpu.CGConfig(preconditioner=JACOBI))
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT, (case, res.error_code)
        assert np.array_equal(d_x.copyToHost(4), x0)
    finally:
        gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------------ reproducibility
def test_two_solves_give_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)           # lets the tiled engine take a small matrix
    n, rp, ci, va = spd.random_spd(50_000, 7, seed=11)
    s = System(gpu, n, rp, ci, va)
    try:
        for engine in (0, 1):
            r1, x1 = s.solve(tolerance=1e-6, engine=engine)
            r2, x2 = s.solve(tolerance=1e-6, engine=engine)
            assert r1.error_code == 0 and r1.converged
            assert r1.iterations == r2.iterations and r1.relative_residual == r2.relative_residual
            assert np.array_equal(x1.view(np.uint32), x2.view(np.uint32)), engine
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ engine parity
def test_engines_agree_on_a_tiled_eligible_matrix(gpu):
    n, rp, ci, va = spd.poisson3d(64)                    # 262 144 columns, 1.8 M entries: tiled-eligible
    assert gpu.tiled_shape(n, n, ci.size)[0]
    tol = 1e-5
    s = System(gpu, n, rp, ci, va)
    try:
        x_ref, it_ref, _, _, _ = restate(n, rp, ci, va, s.b, np.zeros(n), tol)
        bound = max(4 * tol, 2 * true_residual(rp, ci, va, s.b, x_ref))
        iters = {}
        for engine in (0, 1, -1):                          # 1 builds the plan, -1 then finds it cached
            res, x = s.solve(tolerance=tol, engine=engine)
            assert res.error_code == 0 and res.converged and not res.breakdown, engine
            assert true_residual(rp, ci, va, s.b, x) <= bound, engine
            iters[engine] = res.iterations
        assert max(iters.values()) - min(iters.values()) <= max(1, 0.02 * min(iters.values())), iters
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        s.close()


def test_auto_engine_builds_and_caches_a_plan_and_leaves_promotion_alone(gpu):
    n, rp, ci, va = spd.poisson3d(64)
    s = System(gpu, n, rp, ci, va)
    saved = gpu.get_tiled_promotion()
    try:
        # solves never count toward promotion: after them, VECTOR_CSR calls promote exactly as on a fresh matrix
        gpu.set_tiled_promotion(2)
        for _ in range(3):
            res0, _ = s.solve(tolerance=1e-5, engine=0)
            assert res0.converged
        assert not gpu.csr_has_tiled_plan(s.A)              # engine 0 never builds a plan
        d_y = gpu.CudaBuffer(n)
        for call in range(3):
            assert gpu.spmv_csr(s.A, s.d_b, d_y, gpu.SpMVConfig(1), n).error_code == 0
            assert gpu.csr_has_tiled_plan(s.A) == (call >= 2), call
        d_y.release()
        # auto: no plan cached -> 4 direct steps, then a plan that stays with A
        gpu.csr_invalidate_gpu_cache(s.A)
        res, _ = s.solve(tolerance=1e-5, engine=-1)
        assert res.converged and res.iterations > 4
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        gpu.set_tiled_promotion(saved)
        s.close()


# ------------------------------------------------------------------------------------------ run-ahead
def test_steps_enqueued_after_done_change_nothing(gpu):
    n, rp, ci, va = spd.poisson2d(64)
    s = System(gpu, n, rp, ci, va)
    try:
        tol = 1e-5
        _, it_ref, _, _, _ = restate(n, rp, ci, va, s.b, np.zeros(n), tol)
        res, x = s.solve(tolerance=tol, engine=0)
        assert res.converged and abs(res.iterations - it_ref) <= 2
        # the same solve stopped by max_iterations at the reported count: no step past `done` moved x
        res_k, x_k = s.solve(tolerance=tol, engine=0, max_iterations=res.iterations)
        assert res_k.iterations == res.iterations and res_k.converged
        assert np.array_equal(x.view(np.uint32), x_k.view(np.uint32))
        res_k1, x_k1 = s.solve(tolerance=tol, engine=0, max_iterations=res.iterations + 1)
        assert np.array_equal(x.view(np.uint32), x_k1.view(np.uint32)) and res_k1.iterations == res.iterations
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_cg_smoke(gpu, tmp_path):
    """tests/cpp/cg_smoke.cpp through spmv/cg.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "cg_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "cg_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
