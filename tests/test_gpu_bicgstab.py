"""bicgstab_solve (include/spmv/bicgstab.h) on the device.

The solver is checked against a numpy restatement that follows the documented numerics (fp32 vectors, fp64 dot
products of the fp32 entries, alpha, omega and beta rounded to fp32 and applied as multiply-adds, p^ = p * dinv and
s^ = s * dinv, the half-step test on ||s|| and the stop test on ||r||, the three breakdown codes), against small
systems whose every step is exact in fp32, for its argument rejections on the device, for run-to-run
reproducibility, for agreement between its engines and with cg_solve, and through a C++ caller.

BiCGSTAB is far more sensitive to rounding than CG: reordering the fp32 sums of the SpMV alone (numpy's sequential
row sums against fp64 sums rounded once) moves the converged iteration count by up to 4 % and the final residual by
tens of per cent on the convection-diffusion matrices, while after 10 steps the residuals still agree to 1e-5 %.
The device's own summation order (lanes of the vector-CSR kernel, then a butterfly) is a third order: on the
MI355X it ends convdiff2d_64_mild (JACOBI, 1e-4) 6.5 % before the restatement.  So the converged solves are compared
on iterations (to 10 %), flags and residual bounds, and the residual itself to 1 % at fixed step counts."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
NONE, JACOBI = 0, 1
NO_BREAKDOWN, RHO, ALPHA, OMEGA = 0, 1, 2, 3
TILED_SMALL = "min_cols=1,min_nnz=1"


# ------------------------------------------------------------------------------------------ restatement
def diag_of(n, rp, ci, va):
    """fp32 sum of the stored (i,i) entries in storage order (0 where a row has none)"""
    d = np.zeros(n, np.float32)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))
    for j in np.flatnonzero(ci == rows):
        d[rows[j]] = np.float32(d[rows[j]] + va[j])
    return d


def spmv32(rp, ci, va, x):
    return spd.spmv64(rp, ci, va, x).astype(np.float32)


def fma(a, u, c):
    """fp32 fmaf(a, u, c) elementwise (the product of two fp32 values is exact in fp64)"""
    return (np.float64(a) * u.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def usable(v):
    return v != 0 and np.isfinite(v)


def restate(n, rp, ci, va, b, x0, tol, max_iter=1000, precond=JACOBI):
    """numpy BiCGSTAB under bicgstab.h's rules; returns (x, iterations, converged, breakdown, relative residual)"""
    dot = lambda a, c: np.float64(np.dot(a.astype(np.float64), c.astype(np.float64)))
    b = np.asarray(b, np.float32)
    x = np.asarray(x0, np.float32).copy()
    dinv = (np.float32(1.0) / diag_of(n, rp, ci, va)).astype(np.float32) if precond == JACOBI else None
    pre = (lambda u: (u * dinv).astype(np.float32)) if dinv is not None else (lambda u: u)
    r = (b - spmv32(rp, ci, va, x)).astype(np.float32)
    rhat, p = r.copy(), r.copy()
    rr, bb = dot(r, r), dot(b, b)
    if bb == 0:
        return np.zeros(n, np.float32), 0, True, NO_BREAKDOWN, 0.0
    bnorm = np.sqrt(bb)
    thr = np.float64(np.float32(tol)) * bnorm
    rel = np.sqrt(rr) / bnorm
    if np.sqrt(rr) <= thr:
        return x, 0, True, NO_BREAKDOWN, rel
    if not usable(rr):
        return x, 0, False, RHO, rel
    rho = rr
    with np.errstate(all="ignore"):
        for k in range(max_iter):
            ph = pre(p)
            v = spmv32(rp, ci, va, ph)
            rv = dot(rhat, v)
            if not usable(rv):
                return x, k, False, ALPHA, rel
            a = np.float32(rho / rv)
            s = fma(-a, v, r)
            sres = np.sqrt(dot(s, s))
            sh = pre(s)
            t = spmv32(rp, ci, va, sh)
            if sres <= thr:
                return fma(a, ph, x), k + 1, True, NO_BREAKDOWN, sres / bnorm
            w = np.float32(dot(t, s) / dot(t, t))
            if not usable(w):
                if np.isfinite(sres):
                    return fma(a, ph, x), k + 1, False, OMEGA, sres / bnorm
                return x, k, False, OMEGA, sres / bnorm
            x = fma(w, sh, fma(a, ph, x))
            r = fma(-w, t, s)
            rr, rho_new = dot(r, r), dot(rhat, r)
            rel = np.sqrt(rr) / bnorm
            if np.sqrt(rr) <= thr:
                return x, k + 1, True, NO_BREAKDOWN, rel
            if not usable(rho_new):
                return x, k + 1, False, RHO, rel
            beta = np.float32((rho_new / rho) * (np.float64(a) / np.float64(w)))
            p = fma(beta, fma(-w, v, p), r)
            rho = rho_new
    return x, max_iter, False, NO_BREAKDOWN, rel


def true_residual(rp, ci, va, b, x):
    b64 = np.asarray(b, np.float64)
    return float(np.linalg.norm(b64 - spd.spmv64(rp, ci, va, x)) / np.linalg.norm(b64))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class System:
    """A matrix on the device (csr_from_arrays + csr_to_gpu) with device b and x buffers."""

    def __init__(self, gpu, n, rp, ci, va, seed=1, b=None):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        rng = np.random.default_rng(seed)
        self.b = rng.uniform(-1.0, 1.0, n).astype(np.float32) if b is None else np.asarray(b, np.float32)
        self.d_b = gpu.CudaBuffer(n)
        self.d_x = gpu.CudaBuffer(n)
        self.d_b.copyFromHost(self.b, n)

    def _run(self, solver, config, x0):
        x0 = np.zeros(self.n, np.float32) if x0 is None else np.asarray(x0, np.float32)
        self.d_x.copyFromHost(x0, self.n)
        res = solver(self.A, self.d_b, self.d_x, config)
        return res, self.d_x.copyToHost(self.n)

    def solve(self, x0=None, **cfg):
        return self._run(self.gpu.bicgstab_solve, self.gpu.BiCGStabConfig(**cfg), x0)

    def cg(self, x0=None, **cfg):
        return self._run(self.gpu.cg_solve, self.gpu.CGConfig(**cfg), x0)

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def dense_csr(dense):
    dense = np.asarray(dense, np.float32)
    n = dense.shape[0]
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, cols.astype(np.int32), dense[rows, cols]


MATRICES = {
    "convdiff2d_64_mild": lambda: nonsym.convdiff2d(64, 1.0),
    "convdiff2d_64_strong": lambda: nonsym.convdiff2d(64, 50.0),
    "convdiff2d_256": lambda: nonsym.convdiff2d(256, 1.0),
    "random_nonsym_1e5": lambda: nonsym.random_nonsym(100_000, 7, seed=3),
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
                what = (name, precond, tol, res.iterations, it_ref, res.relative_residual, rel_ref)
                assert abs(res.iterations - it_ref) <= max(3, 0.10 * it_ref), what
                assert bool(res.converged) == conv_ref and res.breakdown == brk_ref == NO_BREAKDOWN, what
                assert res.relative_residual <= tol, what
                bound = max(4 * tol, 2 * true_residual(rp, ci, va, s.b, x_ref))
                assert true_residual(rp, ci, va, s.b, x) <= bound, what
                assert res.elapsed_ms > 0
            # where the trajectories have not parted yet: the residual to 1 %, x to 1e-4
            for k in (1, 10):
                res, x = s.solve(tolerance=1e-7, preconditioner=precond, engine=0, max_iterations=k)
                x_ref, it_ref, conv_ref, brk_ref, rel_ref = restate(n, rp, ci, va, s.b, np.zeros(n), 1e-7, k,
                                                                    precond)
                what = (name, precond, k, res.iterations, it_ref, res.relative_residual, rel_ref)
                assert (res.iterations, bool(res.converged), res.breakdown) == (it_ref, conv_ref, brk_ref), what
                assert abs(res.relative_residual - rel_ref) <= 0.01 * rel_ref, what
                err = np.linalg.norm(x.astype(np.float64) - x_ref) / np.linalg.norm(x_ref.astype(np.float64))
                assert err <= 1e-4, (what, err)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ exact known answers
# Integer systems whose every alpha and omega is dyadic: each step is exact in fp32, so every bit is known.
# (A, b, breakdown, iterations, x, relative residual), solved with NONE from x0 = 0.
KNOWN = {
    "alpha": ([[0, 1], [-1, 0]], [1, 0], ALPHA, 0, [0, 0], 1.0),
    "omega": ([[-2, -2], [-2, 0]], [-2, 0], OMEGA, 1, [1, 0], 1.0),
    "rho": ([[-1, -1, -1], [-1, -1, 0], [0, -1, -1]], [0, 0, -1], RHO, 1, [-0.5, 0, 1], np.sqrt(0.5)),
}


@pytest.mark.parametrize("case", list(KNOWN))
def test_exact_breakdowns(gpu, case):
    dense, b, brk, iters, x_want, rel = KNOWN[case]
    n, rp, ci, va = dense_csr(dense)
    s = System(gpu, n, rp, ci, va, b=b)
    try:
        x_ref, it_ref, conv_ref, brk_ref, _ = restate(n, rp, ci, va, s.b, np.zeros(n), 1e-6, 1000, NONE)
        assert (it_ref, conv_ref, brk_ref) == (iters, False, brk) and np.array_equal(bits(x_ref), bits(x_want))
        for engine in (0, 1):                       # engine 1 runs the direct kernels here (not tiled-eligible)
            res, x = s.solve(tolerance=1e-6, preconditioner=NONE, engine=engine)
            assert (res.error_code, res.converged, res.breakdown, res.iterations) == (0, 0, brk, iters), case
            assert np.array_equal(bits(x), bits(x_want)), (case, x)
            assert res.relative_residual == np.float32(rel), (case, res.relative_residual)
    finally:
        s.close()


def test_signed_power_of_two_diagonal_converges_at_the_half_step(gpu):
    n = 1000
    rng = np.random.default_rng(5)
    d = np.ldexp(np.float32(1.0), rng.integers(-3, 6, n)).astype(np.float32)
    d[rng.random(n) < 0.5] *= -1                                        # negative diagonals are allowed
    rp = np.arange(n + 1, dtype=np.int32)
    ci = np.arange(n, dtype=np.int32)
    s = System(gpu, n, rp, ci, d)
    try:
        res, x = s.solve(tolerance=1e-6, preconditioner=JACOBI, engine=0)
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 1, NO_BREAKDOWN)
        assert res.relative_residual == 0.0
        want = (s.b * (np.float32(1.0) / d).astype(np.float32)).astype(np.float32)    # b * dinv
        assert np.array_equal(bits(x), bits(want))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ negative diagonals
def test_negative_diagonals_converge_under_jacobi_and_cg_rejects_them(gpu):
    n, rp, ci, va = nonsym.random_nonsym(100_000, 7, seed=4, negative_rows=0.5)
    assert (diag_of(n, rp, ci, va) < 0).mean() > 0.4
    tol = 1e-5
    s = System(gpu, n, rp, ci, va)
    try:
        res, x = s.solve(tolerance=tol, preconditioner=JACOBI, engine=0)
        assert res.error_code == 0 and res.converged and res.breakdown == NO_BREAKDOWN
        x_ref, it_ref, _, _, _ = restate(n, rp, ci, va, s.b, np.zeros(n), tol)
        assert abs(res.iterations - it_ref) <= 3
        assert true_residual(rp, ci, va, s.b, x) <= max(4 * tol, 2 * true_residual(rp, ci, va, s.b, x_ref))
        x0 = np.full(n, 0.25, np.float32)
        res_cg, x_cg = s.cg(x0=x0, preconditioner=JACOBI)
        assert res_cg.error_code == gpu.SpMVError.INVALID_ARGUMENT
        assert np.array_equal(x_cg, x0)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ SPD cross-check
def test_agrees_with_cg_on_an_spd_matrix(gpu):
    n, rp, ci, va = spd.poisson2d(64)
    tol = 1e-6
    s = System(gpu, n, rp, ci, va)
    try:
        res_cg, x_cg = s.cg(tolerance=tol, preconditioner=JACOBI, engine=0)
        assert res_cg.converged
        for precond in (NONE, JACOBI):
            res, x = s.solve(tolerance=tol, preconditioner=precond, engine=0)
            assert res.error_code == 0 and res.converged and res.breakdown == NO_BREAKDOWN
            diff = np.linalg.norm(x.astype(np.float64) - x_cg) / np.linalg.norm(x_cg.astype(np.float64))
            assert diff <= 2e-4, (precond, diff)                  # the restatements differ by 3e-5
            assert true_residual(rp, ci, va, s.b, x) <= 20 * tol
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("case", ["zero", "nan", "missing"])
def test_jacobi_rejects_a_bad_diagonal_and_leaves_x_untouched(gpu, case):
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, -3, 0, 1, 1, 5]
    elif case == "nan":                         # (2,2) = NaN
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [4, .5, .5, -3, np.nan, 5]
    else:                                       # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [4, .5, .5, -3, 1, 1]
    A = gpu.csr_from_arrays(4, 4, rp, ci, np.asarray(va, np.float32))
    assert gpu.csr_to_gpu(A) == 0
    d_b, d_x = gpu.CudaBuffer(4), gpu.CudaBuffer(4)
    d_b.copyFromHost(np.ones(4, np.float32), 4)
    x0 = np.array([7.0, -1.0, 2.5, 0.25], np.float32)
    d_x.copyFromHost(x0, 4)
    try:
        res = gpu.bicgstab_solve(A, d_b, d_x, gpu.BiCGStabConfig(preconditioner=JACOBI))
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT, (case, res.error_code)
        assert np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
    finally:
        gpu.csr_destroy(A)
        d_b.release()
        d_x.release()


def test_zero_b_writes_zeros(gpu):
    n, rp, ci, va = nonsym.convdiff2d(16, 2.0)
    s = System(gpu, n, rp, ci, va, b=np.zeros(n, np.float32))
    try:
        res, x = s.solve(x0=np.full(n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(n, np.float32))
    finally:
        s.close()


def test_good_initial_guess_returns_at_once_and_leaves_x_alone(gpu):
    n, rp, ci, va = nonsym.convdiff2d(32, 2.0)
    s = System(gpu, n, rp, ci, va)
    try:
        res, x_solved = s.solve(tolerance=1e-5)
        assert res.converged and res.iterations > 0
        res2, x2 = s.solve(x0=x_solved, tolerance=1e-3)
        assert (res2.error_code, res2.converged, res2.iterations, res2.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(bits(x2), bits(x_solved))
        assert res2.relative_residual <= 1e-3
    finally:
        s.close()


def test_max_iterations_stops_there(gpu):
    n, rp, ci, va = nonsym.convdiff2d(64, 5.0)
    s = System(gpu, n, rp, ci, va)
    try:
        for precond in (NONE, JACOBI):
            for k in (1, 5, 20):
                res, x = s.solve(tolerance=1e-7, max_iterations=k, preconditioner=precond, engine=0)
                assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
        res, x = s.solve(max_iterations=0, x0=np.full(n, 0.5, np.float32))
        assert (res.error_code, res.iterations, res.converged) == (0, 0, 0)
        assert np.all(x == np.float32(0.5))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ reproducibility
def test_two_solves_give_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)           # lets the tiled engine take a small matrix
    n, rp, ci, va = nonsym.random_nonsym(50_000, 7, seed=11, negative_rows=0.25)
    s = System(gpu, n, rp, ci, va)
    try:
        for engine in (0, 1):
            for precond in (NONE, JACOBI):
                r1, x1 = s.solve(tolerance=1e-6, engine=engine, preconditioner=precond)
                r2, x2 = s.solve(tolerance=1e-6, engine=engine, preconditioner=precond)
                assert r1.error_code == 0 and r1.converged, (engine, precond)
                assert (r1.iterations, r1.relative_residual) == (r2.iterations, r2.relative_residual)
                assert np.array_equal(bits(x1), bits(x2)), (engine, precond)
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ engine parity
def test_engines_agree_on_a_tiled_eligible_matrix(gpu):
    n, rp, ci, va = nonsym.convdiff3d(64, 1.0)            # 262 144 columns, 1.8 M entries: tiled-eligible
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
        assert max(iters.values()) - min(iters.values()) <= max(3, 0.05 * min(iters.values())), iters
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        s.close()


def test_auto_engine_builds_and_caches_a_plan_and_leaves_promotion_alone(gpu):
    n, rp, ci, va = nonsym.convdiff3d(64, 1.0)
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
@pytest.mark.parametrize("precond", [NONE, JACOBI])
def test_steps_enqueued_after_done_change_nothing(gpu, precond):
    n, rp, ci, va = nonsym.convdiff2d(64, 1.0)
    s = System(gpu, n, rp, ci, va)
    try:
        tol = 1e-5
        res, x = s.solve(tolerance=tol, engine=0, preconditioner=precond)
        assert res.converged
        # the same solve stopped by max_iterations at the reported count: no step past `done` moved x
        res_k, x_k = s.solve(tolerance=tol, engine=0, preconditioner=precond, max_iterations=res.iterations)
        assert res_k.iterations == res.iterations and res_k.converged
        assert np.array_equal(bits(x), bits(x_k))
        res_k1, x_k1 = s.solve(tolerance=tol, engine=0, preconditioner=precond, max_iterations=res.iterations + 1)
        assert np.array_equal(bits(x), bits(x_k1)) and res_k1.iterations == res.iterations
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_bicgstab_smoke(gpu, tmp_path):
    """tests/cpp/bicgstab_smoke.cpp through spmv/bicgstab.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "bicgstab_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "bicgstab_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
