"""bicgstab_solve_lu (include/spmv/bicgstab.h) on the device, preconditioned by the ILU(0) factor of ilu0_csr.

Checked against a numpy restatement of the documented iteration (test_gpu_bicgstab.py's scheme, with p^ and s^ from
sptrsv_cpu_csr on the factor) by the project's residual bound; for the iteration counts against Jacobi that are the
reason the preconditioner exists; on an exact factor, where the preconditioned solve is a direct one; for
reproducibility, engine agreement, the stop rules it shares with bicgstab_solve, its rejections, and through a C++
caller.  The restatement's triangular solves sum in storage order with separate roundings while the device's use
1-64 lanes and fused multiply-adds, so trajectories are compared by bounds, never bit for bit."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ilu0_cases as cases
import test_gpu_bicgstab as base
from conftest import ROOT
from test_gpu_bicgstab import bits, fma, spmv32, true_residual, usable

pytestmark = pytest.mark.gpu

nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
NO_BREAKDOWN, RHO, ALPHA, OMEGA = 0, 1, 2, 3
JACOBI = 1
TOL = 1e-6

MATRICES = {
    "convdiff2d(16,1)": lambda: nonsym.convdiff2d(16, 1.0),
    "convdiff2d(24,(3,.5))": lambda: nonsym.convdiff2d(24, (3.0, 0.5)),
    "convdiff3d(8,1)": lambda: nonsym.convdiff3d(8, 1.0),
}


class LUSystem(base.System):
    """base.System plus the ILU(0) factor of its matrix on the device, wrapped over A's structure arrays, and the same
    factor as a host matrix for the restatement"""

    def __init__(self, gpu, n, rp, ci, va, seed=1, b=None):
        super().__init__(gpu, n, rp, ci, va, seed=seed, b=b)
        self.d_lu = gpu.CudaBuffer(ci.size)
        res = gpu.ilu0_csr(self.A, self.d_lu)
        assert res.error_code == 0 and res.zero_pivot == -1
        self.lu = self.d_lu.copyToHost(ci.size)
        np.testing.assert_array_equal(bits(self.lu), bits(gpu.ilu0_cpu_csr(self.A)[0]))
        self.F = gpu.csr_wrap_device(n, n, int(ci.size), self.A.contents.d_row_ptrs, self.A.contents.d_col_indices,
                                     self.d_lu.get())
        self.F_host = gpu.csr_from_arrays(n, n, rp, ci, self.lu)

    def solve_lu(self, x0=None, LU=None, **cfg):
        solver = lambda A, d_b, d_x, config: self.gpu.bicgstab_solve_lu(A, self.F if LU is None else LU, d_b, d_x,
                                                                        config)
        return self._run(solver, self.gpu.BiCGStabConfig(**cfg), x0)

    def precondition(self, u):
        gpu = self.gpu
        y = gpu.sptrsv_cpu_csr(self.F_host, u, gpu.SpTRSVConfig(uplo=0, diag=1))
        return gpu.sptrsv_cpu_csr(self.F_host, y, gpu.SpTRSVConfig(uplo=1, diag=0))

    def close(self):
        self.gpu.csr_destroy(self.F)
        self.gpu.csr_destroy(self.F_host)
        self.d_lu.release()
        super().close()


def restate_lu(s, x0, tol, max_iter=1000):
    """bicgstab.h's iteration with p^ = U^-1 (L^-1 p), s^ = U^-1 (L^-1 s) in numpy;
    (x, iterations, converged, breakdown, relative residual)"""
    rp, ci, va, n = s.rp, s.ci, s.va, s.n
    dot = lambda a, c: np.float64(np.dot(a.astype(np.float64), c.astype(np.float64)))
    b = np.asarray(s.b, np.float32)
    x = np.asarray(x0, np.float32).copy()
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
            ph = s.precondition(p)
            v = spmv32(rp, ci, va, ph)
            rv = dot(rhat, v)
            if not usable(rv):
                return x, k, False, ALPHA, rel
            a = np.float32(rho / rv)
            sv = fma(-a, v, r)
            sres = np.sqrt(dot(sv, sv))
            if sres <= thr:
                return fma(a, ph, x), k + 1, True, NO_BREAKDOWN, sres / bnorm
            sh = s.precondition(sv)
            t = spmv32(rp, ci, va, sh)
            w = np.float32(dot(t, sv) / dot(t, t))
            if not usable(w):
                if np.isfinite(sres):
                    return fma(a, ph, x), k + 1, False, OMEGA, sres / bnorm
                return x, k, False, OMEGA, sres / bnorm
            x = fma(w, sh, fma(a, ph, x))
            r = fma(-w, t, sv)
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


@pytest.fixture(scope="module")
def systems(gpu):
    """the three convection-diffusion systems with their factors and the restatement's answer, computed once"""
    built = {}
    for name, make in MATRICES.items():
        s = LUSystem(gpu, *make())
        built[name] = (s, restate_lu(s, np.zeros(s.n), TOL))
    yield built
    for s, _ in built.values():
        s.close()


# ------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", list(MATRICES))
def test_restatement_parity(gpu, systems, name):
    s, (x_ref, it_ref, conv_ref, brk_ref, rel_ref) = systems[name]
    assert conv_ref and brk_ref == NO_BREAKDOWN
    res, x = s.solve_lu(tolerance=TOL, engine=0)
    what = (name, res.iterations, it_ref, res.relative_residual, rel_ref)
    print("bicgstab_solve_lu", what)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    assert res.converged == 1 and res.breakdown == NO_BREAKDOWN, what
    bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
    assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, what
    if res.iterations == it_ref:
        assert abs(res.relative_residual - rel_ref) <= 0.01 * rel_ref, what
    assert res.elapsed_ms > 0
    # the preconditioner field is not read
    res2, x2 = s.solve_lu(tolerance=TOL, engine=0, preconditioner=2)
    assert (res2.error_code, res2.iterations) == (0, res.iterations) and np.array_equal(bits(x2), bits(x))


# ------------------------------------------------------------------------------------------ against Jacobi
@pytest.mark.parametrize("name", list(MATRICES))
def test_at_most_half_the_iterations_of_jacobi(gpu, systems, name):
    """A condition on the inputs: the CPU restatement gives 7 / 24, 7 / 34 and 5 / 16."""
    s, _ = systems[name]
    lu, _ = s.solve_lu(tolerance=TOL, engine=0)
    jacobi, _ = s.solve(tolerance=TOL, engine=0, preconditioner=JACOBI)
    print(f"{name}: ILU(0) {lu.iterations} iterations, Jacobi {jacobi.iterations}")
    assert lu.error_code == 0 and lu.converged and jacobi.error_code == 0 and jacobi.converged
    assert 2 * lu.iterations <= jacobi.iterations, (name, lu.iterations, jacobi.iterations)


# ------------------------------------------------------------------------------------------ exact factor
def test_an_exact_factor_is_a_direct_solve(gpu):
    n, rp, ci, va, fact = cases.exact_tridiagonal(257, lower=-1, diag=4, upper=-2)
    np.testing.assert_array_equal(bits(cases.prove_exact(n, rp, ci, va)), bits(fact))
    for seed in (1, 2, 3):
        s = LUSystem(gpu, n, rp, ci, va, seed=seed)
        try:
            np.testing.assert_array_equal(bits(s.lu), bits(fact))
            res, x = s.solve_lu(tolerance=1e-4, engine=0)
            residual = true_residual(rp, ci, va, s.b, x)
            print(f"exact factor, seed {seed}: {res.iterations} iteration(s), true residual {residual:.3g}")
            assert (res.error_code, res.converged, res.breakdown, res.iterations) == (0, 1, 0, 1)
            assert residual < 1e-6
        finally:
            s.close()


# ------------------------------------------------------------------------------------------ reproducibility, engines
def test_two_solves_give_the_same_bits(gpu, systems):
    for name, (s, _) in systems.items():
        r1, x1 = s.solve_lu(tolerance=TOL, engine=0)
        r2, x2 = s.solve_lu(tolerance=TOL, engine=0)
        assert r1.error_code == 0 and r1.converged, name
        assert (r1.iterations, r1.relative_residual) == (r2.iterations, r2.relative_residual), name
        assert np.array_equal(bits(x1), bits(x2)), name


def test_engines_agree_on_a_tiled_eligible_matrix(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", base.TILED_SMALL)          # lets the tiled engine take a small matrix
    s = LUSystem(gpu, *nonsym.convdiff2d(64, 1.0))
    try:
        x_ref, it_ref, conv_ref, _, _ = restate_lu(s, np.zeros(s.n), TOL)
        assert conv_ref
        bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
        iters = {}
        for engine in (0, 1):
            res, x = s.solve_lu(tolerance=TOL, engine=engine)
            assert res.error_code == 0 and res.converged and not res.breakdown, engine
            assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, engine
            assert gpu.csr_has_tiled_plan(s.A) == (engine == 1)
            iters[engine] = res.iterations
        assert abs(iters[0] - iters[1]) <= 3, iters
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ stop rules
def test_max_iterations_stops_there_and_steps_after_done_change_nothing(gpu, systems):
    s, _ = systems["convdiff2d(24,(3,.5))"]
    full, x_full = s.solve_lu(tolerance=TOL, engine=0)
    assert full.converged and full.iterations >= 3
    for k in (1, 2):
        res, _ = s.solve_lu(tolerance=TOL, engine=0, max_iterations=k)
        assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
    res, x = s.solve_lu(max_iterations=0, x0=np.full(s.n, 0.5, np.float32))
    assert (res.error_code, res.iterations, res.converged) == (0, 0, 0) and np.all(x == np.float32(0.5))
    # stopped by max_iterations at the reported count, and one past it: no step past `done` moved x
    for extra in (0, 1):
        res_k, x_k = s.solve_lu(tolerance=TOL, engine=0, max_iterations=full.iterations + extra)
        assert res_k.iterations == full.iterations and res_k.converged
        assert np.array_equal(bits(x_k), bits(x_full))


def test_zero_b_writes_zeros(gpu):
    s = LUSystem(gpu, *nonsym.convdiff2d(16, 2.0), b=np.zeros(256, np.float32))
    try:
        res, x = s.solve_lu(x0=np.full(s.n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(s.n, np.float32))
    finally:
        s.close()


def test_good_initial_guess_returns_at_once_and_leaves_x_alone(gpu, systems):
    s, _ = systems["convdiff2d(16,1)"]
    res, x_solved = s.solve_lu(tolerance=1e-5)
    assert res.converged and res.iterations > 0
    res2, x2 = s.solve_lu(x0=x_solved, tolerance=1e-3)
    assert (res2.error_code, res2.converged, res2.iterations, res2.breakdown) == (0, 1, 0, 0)
    assert np.array_equal(bits(x2), bits(x_solved)) and res2.relative_residual <= 1e-3


# ------------------------------------------------------------------------------------------ rejections
@pytest.mark.parametrize("case", ["zero", "nan", "missing"])
def test_a_bad_factor_diagonal_is_rejected_and_x_is_untouched(gpu, case):
    a_rp, a_ci, a_va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, -3, 2, 1, 1, 5]
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = a_rp, a_ci, [4, .5, .5, -3, 0, 1, 1, 5]
    elif case == "nan":                         # (2,2) = NaN
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [4, .5, .5, -3, np.nan, 5]
    else:                                       # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [4, .5, .5, -3, 1, 1]
    A = gpu.csr_from_arrays(4, 4, a_rp, a_ci, np.asarray(a_va, np.float32))
    F = gpu.csr_from_arrays(4, 4, rp, ci, np.asarray(va, np.float32))          # a pattern of its own
    assert gpu.csr_to_gpu(A) == 0 and gpu.csr_to_gpu(F) == 0
    d_b, d_x = gpu.CudaBuffer(4), gpu.CudaBuffer(4)
    d_b.copyFromHost(np.ones(4, np.float32), 4)
    x0 = np.array([7.0, -1.0, 2.5, 0.25], np.float32)
    d_x.copyFromHost(x0, 4)
    try:
        res = gpu.bicgstab_solve_lu(A, F, d_b, d_x, gpu.BiCGStabConfig(preconditioner=0))
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT, (case, res.error_code)
        assert np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
        # the same A with itself as the factor is fine (its diagonal is sound), and x moves
        assert gpu.bicgstab_solve_lu(A, A, d_b, d_x).error_code == 0
        assert not np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(F)
        d_b.release()
        d_x.release()


def test_a_factor_of_another_size_and_an_unknown_preconditioner_of_bicgstab_solve(gpu, systems):
    E = gpu.SpMVError
    s, _ = systems["convdiff2d(16,1)"]
    other, _ = systems["convdiff3d(8,1)"]
    x0 = np.full(s.n, 0.25, np.float32)
    res, x = s.solve_lu(x0=x0, LU=other.F)
    assert res.error_code == E.INVALID_DIMENSION and np.array_equal(bits(x), bits(x0))
    # malformed structure of the factor: INVALID_FORMAT from the analysis, x untouched
    bad_ci = s.ci.copy()
    bad_ci[5] = s.n + 3
    B = gpu.csr_from_arrays(s.n, s.n, s.rp, bad_ci, s.va)
    assert gpu.csr_to_gpu(B) == 0
    res, x = s.solve_lu(x0=x0, LU=B)
    assert res.error_code == E.INVALID_FORMAT and np.array_equal(bits(x), bits(x0))
    gpu.csr_destroy(B)
    # bicgstab_solve keeps rejecting a preconditioner value it does not know
    res, x = s.solve(x0=x0, preconditioner=2)
    assert res.error_code == E.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_ilu0_smoke(gpu, tmp_path):
    """tests/cpp/ilu0_smoke.cpp through spmv/ilu0.h, spmv/bicgstab.h and CudaBuffer, compiled here with build()'s g++
    line."""
    exe = str(tmp_path / "ilu0_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "ilu0_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
