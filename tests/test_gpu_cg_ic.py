"""cg_solve_ic (include/spmv/cg.h) on the device, preconditioned by the IC(0) factor of ic0_csr.

Checked against a numpy restatement of the documented iteration (test_gpu_cg.py's scheme, with z from sptrsv_cpu_csr
on the host factor) by the project's residual bound; for the iteration counts against Jacobi that are the reason the
preconditioner exists; on an exact factor, where the preconditioned solve is a direct one; for reproducibility, engine
agreement, the stop rules it shares with cg_solve, a breakdown, its rejections, and through a C++ caller.  The
restatement's triangular solves sum in storage order with separate roundings while the device's use 1-64 lanes and
fused multiply-adds, so trajectories are compared by bounds, never bit for bit."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ic0_cases as cases
import test_gpu_bicgstab as base
from conftest import ROOT
from test_gpu_bicgstab import bits, fma, spmv32, true_residual

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
JACOBI = 1
TOL = 1e-6

MATRICES = {
    "poisson2d(16)": lambda: spd.poisson2d(16),
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
}


class ICSystem(base.System):
    """base.System plus the IC(0) factor of its matrix on the device, wrapped over A's structure arrays, and the same
    factor as a host matrix for the restatement"""

    def __init__(self, gpu, n, rp, ci, va, seed=1, b=None, factor_of=None):
        super().__init__(gpu, n, rp, ci, va, seed=seed, b=b)
        self.d_l = gpu.CudaBuffer(ci.size)
        if factor_of is None:
            res = gpu.ic0_csr(self.A, self.d_l)
        else:                                   # the factor of another matrix on the same pattern
            other = gpu.csr_from_arrays(n, n, rp, ci, factor_of)
            assert gpu.csr_to_gpu(other) == 0
            res = gpu.ic0_csr(other, self.d_l)
            gpu.csr_destroy(other)
        assert res.error_code == 0 and res.bad_pivot == -1
        self.l = self.d_l.copyToHost(ci.size)
        host = gpu.csr_from_arrays(n, n, rp, ci, va if factor_of is None else factor_of)
        np.testing.assert_array_equal(bits(self.l), bits(gpu.ic0_cpu_csr(host)[0]))
        gpu.csr_destroy(host)
        self.F = gpu.csr_wrap_device(n, n, int(ci.size), self.A.contents.d_row_ptrs, self.A.contents.d_col_indices,
                                     self.d_l.get())
        self.F_host = gpu.csr_from_arrays(n, n, rp, ci, self.l)

    def solve_ic(self, x0=None, F=None, **cfg):
        solver = lambda A, d_b, d_x, config: self.gpu.cg_solve_ic(A, self.F if F is None else F, d_b, d_x, config)
        return self._run(solver, self.gpu.CGConfig(**cfg), x0)

    def precondition(self, u):
        gpu = self.gpu
        y = gpu.sptrsv_cpu_csr(self.F_host, u, gpu.SpTRSVConfig(uplo=0, diag=0))
        return gpu.sptrsv_cpu_csr(self.F_host, y, gpu.SpTRSVConfig(uplo=1, diag=0))

    def close(self):
        self.gpu.csr_destroy(self.F)
        self.gpu.csr_destroy(self.F_host)
        self.d_l.release()
        super().close()


def restate_ic(s, x0, tol, max_iter=1000):
    """cg.h's cg_solve_ic iteration with z = L^-T (L^-1 r) in numpy; (x, iterations, converged, breakdown, relative
    residual)"""
    rp, ci, va, n = s.rp, s.ci, s.va, s.n
    dot = lambda a, c: float(np.dot(a.astype(np.float64), c.astype(np.float64)))
    b = np.asarray(s.b, np.float32)
    x = np.asarray(x0, np.float32).copy()
    r = (b - spmv32(rp, ci, va, x)).astype(np.float32)
    z = s.precondition(r)
    p = z.copy()
    rz, rr, bb = dot(r, z), dot(r, r), dot(b, b)
    if bb == 0.0:
        return np.zeros(n, np.float32), 0, True, False, 0.0
    bnorm = np.sqrt(bb)
    thr = float(np.float32(tol)) * bnorm
    rel = np.sqrt(rr) / bnorm
    if np.sqrt(rr) <= thr:
        return x, 0, True, False, rel
    if not rz > 0:
        return x, 0, False, True, rel
    for k in range(max_iter):
        q = spmv32(rp, ci, va, p)
        pq = dot(p, q)
        if not pq > 0:
            return x, k, False, True, rel
        a = np.float32(rz / pq)
        x = fma(a, p, x)
        r = fma(-a, q, r)
        rr = dot(r, r)
        rel = np.sqrt(rr) / bnorm
        if np.sqrt(rr) <= thr:
            return x, k + 1, True, False, rel
        z = s.precondition(r)
        rz_new = dot(r, z)
        if not rz_new > 0:
            return x, k + 1, False, True, rel
        p = fma(np.float32(rz_new / rz), p, z)
        rz = rz_new
    return x, max_iter, False, False, rel


@pytest.fixture(scope="module")
def systems(gpu):
    """the three Poisson systems with their factors and the restatement's answer, computed once"""
    built = {}
    for name, make in MATRICES.items():
        s = ICSystem(gpu, *make())
        built[name] = (s, restate_ic(s, np.zeros(s.n), TOL))
    yield built
    for s, _ in built.values():
        s.close()


# ------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", list(MATRICES))
def test_restatement_parity(gpu, systems, name):
    s, (x_ref, it_ref, conv_ref, brk_ref, rel_ref) = systems[name]
    assert conv_ref and not brk_ref
    res, x = s.solve_ic(tolerance=TOL, engine=0)
    what = (name, res.iterations, it_ref, res.relative_residual, rel_ref)
    print("cg_solve_ic", what)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    assert res.converged == 1 and res.breakdown == 0, what
    bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
    assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, what
    assert res.elapsed_ms > 0
    # the preconditioner field is not read
    res2, x2 = s.solve_ic(tolerance=TOL, engine=0, preconditioner=2)
    assert (res2.error_code, res2.iterations) == (0, res.iterations) and np.array_equal(bits(x2), bits(x))


# ------------------------------------------------------------------------------------------ against Jacobi
@pytest.mark.parametrize("name", list(MATRICES))
def test_at_most_half_the_iterations_of_jacobi(gpu, systems, name):
    """A condition on the inputs: the CPU restatement gives 16 / 44, 23 / 64 and 11 / 27."""
    s, _ = systems[name]
    ic, _ = s.solve_ic(tolerance=TOL, engine=0)
    jacobi, _ = s.cg(tolerance=TOL, engine=0, preconditioner=JACOBI)
    print(f"{name}: IC(0) {ic.iterations} iterations, Jacobi {jacobi.iterations}")
    assert ic.error_code == 0 and ic.converged and jacobi.error_code == 0 and jacobi.converged
    assert 2 * ic.iterations <= jacobi.iterations, (name, ic.iterations, jacobi.iterations)


# ------------------------------------------------------------------------------------------ exact factor
def test_an_exact_factor_is_a_direct_solve(gpu):
    n, rp, ci, va, fact = cases.exact_tridiagonal(257)
    np.testing.assert_array_equal(bits(cases.prove_exact(n, rp, ci, va)), bits(fact))
    for seed in (1, 2, 3):
        s = ICSystem(gpu, n, rp, ci, va, seed=seed)
        try:
            np.testing.assert_array_equal(bits(s.l), bits(fact))
            res, x = s.solve_ic(tolerance=1e-4, engine=0)
            residual = true_residual(rp, ci, va, s.b, x)
            print(f"exact factor, seed {seed}: {res.iterations} iteration(s), true residual {residual:.3g}")
            assert (res.error_code, res.converged, res.breakdown, res.iterations) == (0, 1, 0, 1)
            assert residual < 1e-6
        finally:
            s.close()


# ------------------------------------------------------------------------------------------ reproducibility, engines
def test_two_solves_give_the_same_bits(gpu, systems):
    for name, (s, _) in systems.items():
        r1, x1 = s.solve_ic(tolerance=TOL, engine=0)
        r2, x2 = s.solve_ic(tolerance=TOL, engine=0)
        assert r1.error_code == 0 and r1.converged, name
        assert (r1.iterations, r1.relative_residual) == (r2.iterations, r2.relative_residual), name
        assert np.array_equal(bits(x1), bits(x2)), name


def test_engines_agree_on_a_tiled_eligible_matrix(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", base.TILED_SMALL)          # lets the tiled engine take a small matrix
    s = ICSystem(gpu, *spd.poisson2d(64))
    try:
        x_ref, it_ref, conv_ref, _, _ = restate_ic(s, np.zeros(s.n), TOL)
        assert conv_ref
        bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
        iters = {}
        for engine in (0, 1):
            res, x = s.solve_ic(tolerance=TOL, engine=engine)
            assert res.error_code == 0 and res.converged and not res.breakdown, engine
            assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, engine
            assert gpu.csr_has_tiled_plan(s.A) == (engine == 1)
            iters[engine] = res.iterations
        print("poisson2d(64) engines", iters, "restatement", it_ref)
        assert abs(iters[0] - iters[1]) <= 3, iters
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ stop rules
def test_max_iterations_stops_there_and_steps_after_done_change_nothing(gpu, systems):
    s, _ = systems["poisson2d(24)"]
    full, x_full = s.solve_ic(tolerance=TOL, engine=0)
    assert full.converged and full.iterations >= 3
    for k in (1, 2):
        res, _ = s.solve_ic(tolerance=TOL, engine=0, max_iterations=k)
        assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
    res, x = s.solve_ic(max_iterations=0, x0=np.full(s.n, 0.5, np.float32))
    assert (res.error_code, res.iterations, res.converged) == (0, 0, 0) and np.all(x == np.float32(0.5))
    # stopped by max_iterations at the reported count, and one past it: no step past `done` moved x
    for extra in (0, 1):
        res_k, x_k = s.solve_ic(tolerance=TOL, engine=0, max_iterations=full.iterations + extra)
        assert res_k.iterations == full.iterations and res_k.converged
        assert np.array_equal(bits(x_k), bits(x_full))


def test_zero_b_writes_zeros(gpu):
    s = ICSystem(gpu, *spd.poisson2d(16), b=np.zeros(256, np.float32))
    try:
        res, x = s.solve_ic(x0=np.full(s.n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(s.n, np.float32))
    finally:
        s.close()


def test_good_initial_guess_returns_at_once_and_leaves_x_alone(gpu, systems):
    s, _ = systems["poisson2d(16)"]
    res, x_solved = s.solve_ic(tolerance=1e-5)
    assert res.converged and res.iterations > 0
    res2, x2 = s.solve_ic(x0=x_solved, tolerance=1e-3)
    assert (res2.error_code, res2.converged, res2.iterations, res2.breakdown) == (0, 1, 0, 0)
    assert np.array_equal(bits(x2), bits(x_solved)) and res2.relative_residual <= 1e-3


def test_a_negative_definite_matrix_breaks_down_with_finite_x(gpu):
    n, rp, ci, va = spd.poisson2d(16)
    s = ICSystem(gpu, n, rp, ci, -va, factor_of=va)            # A = -poisson2d(16), M from +poisson2d(16)
    try:
        x0 = np.full(n, 0.25, np.float32)
        res, x = s.solve_ic(x0=x0, tolerance=TOL, engine=0)
        assert (res.error_code, res.converged, res.breakdown) == (0, 0, 1)
        assert np.isfinite(x).all() and np.array_equal(bits(x), bits(x0))     # p.q <= 0 at the first step
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ rejections
@pytest.mark.parametrize("case", ["zero", "negative", "nan", "missing"])
def test_a_bad_factor_diagonal_is_rejected_and_x_is_untouched(gpu, case):
    a_rp, a_ci, a_va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, 3, 2, 1, 1, 5]
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = a_rp, a_ci, [2, .25, .25, 1.5, 0, 1, 1, 2]
    elif case == "negative":                    # (1,1) < 0
        rp, ci, va = a_rp, a_ci, [2, .25, .25, -1.5, 1, 1, 1, 2]
    elif case == "nan":                         # (2,2) = NaN
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [2, .25, .25, 1.5, np.nan, 2]
    else:                                       # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [2, .25, .25, 1.5, 1, 1]
    A = gpu.csr_from_arrays(4, 4, a_rp, a_ci, np.asarray(a_va, np.float32))
    F = gpu.csr_from_arrays(4, 4, rp, ci, np.asarray(va, np.float32))          # a pattern of its own
    assert gpu.csr_to_gpu(A) == 0 and gpu.csr_to_gpu(F) == 0
    d_b, d_x = gpu.CudaBuffer(4), gpu.CudaBuffer(4)
    d_b.copyFromHost(np.ones(4, np.float32), 4)
    x0 = np.array([7.0, -1.0, 2.5, 0.25], np.float32)
    d_x.copyFromHost(x0, 4)
    try:
        res = gpu.cg_solve_ic(A, F, d_b, d_x, gpu.CGConfig(preconditioner=0))
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT, (case, res.error_code)
        assert np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
        # the same A with itself as the factor is fine (its diagonal is sound), and x moves
        assert gpu.cg_solve_ic(A, A, d_b, d_x).error_code == 0
        assert not np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(F)
        d_b.release()
        d_x.release()


def test_a_factor_of_another_size_a_malformed_one_and_an_unknown_preconditioner_of_cg_solve(gpu, systems):
    E = gpu.SpMVError
    s, _ = systems["poisson2d(16)"]
    other, _ = systems["poisson3d(8)"]
    x0 = np.full(s.n, 0.25, np.float32)
    res, x = s.solve_ic(x0=x0, F=other.F)
    assert res.error_code == E.INVALID_DIMENSION and np.array_equal(bits(x), bits(x0))
    # malformed structure of the factor: INVALID_FORMAT from the analysis, x untouched
    bad_ci = s.ci.copy()
    bad_ci[5] = s.n + 3
    B = gpu.csr_from_arrays(s.n, s.n, s.rp, bad_ci, s.va)
    assert gpu.csr_to_gpu(B) == 0
    res, x = s.solve_ic(x0=x0, F=B)
    assert res.error_code == E.INVALID_FORMAT and np.array_equal(bits(x), bits(x0))
    gpu.csr_destroy(B)
    # cg_solve keeps rejecting a preconditioner value it does not know
    res, x = s.cg(x0=x0, preconditioner=2)
    assert res.error_code == E.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_ic0_smoke(gpu, tmp_path):
    """tests/cpp/ic0_smoke.cpp through spmv/ic0.h, spmv/sptrsv.h, spmv/cg.h and CudaBuffer, compiled here with
    build()'s g++ line."""
    exe = str(tmp_path / "ic0_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "ic0_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
