"""cg_solve_amg (include/spmv/cg.h) on the device, preconditioned by one V-cycle of the hierarchy amg_setup builds.

Checked against the numpy restatement of the documented iteration (test_gpu_cg_ic.py's restate_ic with z from
amg_cases' fp32 V-cycle on the levels read back) by the project's residual bound and by iteration counts; against
Jacobi-preconditioned cg_solve, the reason the preconditioner exists; on a one-level hierarchy, where the
preconditioned solve is a direct one; for reproducibility, engine agreement, the stop rules it shares with cg_solve, a
cycle that is not positive definite, its rejections, and through a C++ caller.  The restatement's row sums take
another order than the device's lanes, so trajectories are compared by bounds, never bit for bit."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import amg_cases as ac
import test_gpu_bicgstab as base
from conftest import ROOT
from test_gpu_bicgstab import bits, true_residual
from test_gpu_cg_ic import restate_ic

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
JACOBI = 1
TOL = 1e-6

MATRICES = {
    "poisson2d(32)": lambda: spd.poisson2d(32),
    "poisson2d(48)": lambda: spd.poisson2d(48),
    "poisson3d(12)": lambda: spd.poisson3d(12),
}


class AMGSystem(base.System):
    """base.System plus the hierarchy of its matrix, and the levels read back for the restatement"""

    def __init__(self, gpu, n, rp, ci, va, seed=1, b=None, amg=None):
        super().__init__(gpu, n, rp, ci, va, seed=seed, b=b)
        self.amg = amg if amg is not None else gpu.AMGConfig()
        self.res, self.H = gpu.amg_setup(self.A, self.amg)
        assert self.res.error_code == 0 and self.H is not None
        self.levels = []
        for l in range(self.res.levels):
            m, lrp, lci, lva, agg = gpu.amg_level_arrays(self.H, l)
            self.levels.append(dict(n=m, rp=lrp, ci=lci, va=lva, agg=agg, count=gpu.amg_level(self.H, l)[3]))

    def solve_amg(self, x0=None, H="own", **cfg):
        handle = self.H if isinstance(H, str) else H
        solver = lambda A, d_b, d_x, config: self.gpu.cg_solve_amg(A, handle, d_b, d_x, config)
        return self._run(solver, self.gpu.CGConfig(**cfg), x0)

    def precondition(self, u):
        c = self.amg
        return ac.vcycle(self.levels, u, c.jacobi_weight, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps, np.float32)

    def close(self):
        self.gpu.amg_destroy(self.H)
        super().close()


@pytest.fixture(scope="module")
def systems(gpu):
    """the three Poisson systems with their hierarchies and the restatement's answer, computed once"""
    built = {}
    for name, make in MATRICES.items():
        s = AMGSystem(gpu, *make())
        built[name] = (s, restate_ic(s, np.zeros(s.n), TOL))
    yield built
    for s, _ in built.values():
        s.close()


# ------------------------------------------------------------------------------------------ restatement parity
@pytest.mark.parametrize("name", list(MATRICES))
def test_restatement_parity_and_half_the_iterations_of_jacobi(gpu, systems, name):
    s, (x_ref, it_ref, conv_ref, brk_ref, rel_ref) = systems[name]
    assert conv_ref and not brk_ref
    res, x = s.solve_amg(tolerance=TOL, engine=0)
    jacobi, _ = s.cg(tolerance=TOL, engine=0, preconditioner=JACOBI)
    what = (name, res.iterations, it_ref, jacobi.iterations, res.relative_residual, rel_ref)
    print("cg_solve_amg: iterations, restatement's, Jacobi's", what, "levels", [lv["n"] for lv in s.levels])
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    assert res.converged == 1 and res.breakdown == 0, what
    bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
    assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, what
    assert abs(res.iterations - it_ref) <= max(3, 0.1 * it_ref), what
    assert jacobi.error_code == 0 and jacobi.converged
    assert 2 * it_ref <= jacobi.iterations and 2 * res.iterations <= jacobi.iterations, what
    assert res.elapsed_ms > 0
    # the preconditioner field is not read
    res2, x2 = s.solve_amg(tolerance=TOL, engine=0, preconditioner=2)
    assert (res2.error_code, res2.iterations) == (0, res.iterations) and np.array_equal(bits(x2), bits(x))


def test_a_one_level_hierarchy_is_a_direct_solve(gpu):
    for seed in (1, 2, 3):
        s = AMGSystem(gpu, *spd.random_spd(60, 5, seed=seed), seed=seed)
        try:
            assert s.res.levels == 1 and s.res.coarse_solver == 0
            res, x = s.solve_amg(tolerance=1e-5, engine=0)
            residual = true_residual(s.rp, s.ci, s.va, s.b, x)
            print(f"one level, seed {seed}: {res.iterations} iteration(s), true residual {residual:.3g}")
            assert (res.error_code, res.converged, res.breakdown) == (0, 1, 0) and 1 <= res.iterations <= 2
            assert residual < 4e-5
        finally:
            s.close()


# ------------------------------------------------------------------------------------------ reproducibility, engines
def test_two_solves_give_the_same_bits(gpu, systems):
    for name, (s, _) in systems.items():
        r1, x1 = s.solve_amg(tolerance=TOL, engine=0)
        r2, x2 = s.solve_amg(tolerance=TOL, engine=0)
        assert r1.error_code == 0 and r1.converged, name
        assert (r1.iterations, r1.relative_residual) == (r2.iterations, r2.relative_residual), name
        assert np.array_equal(bits(x1), bits(x2)), name


def test_engines_agree_on_a_tiled_eligible_matrix(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", base.TILED_SMALL)          # lets the tiled engine take a small matrix
    s = AMGSystem(gpu, *spd.poisson2d(64))
    try:
        x_ref, it_ref, conv_ref, _, _ = restate_ic(s, np.zeros(s.n), TOL)
        assert conv_ref
        bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
        iters = {}
        for engine in (0, 1, -1):                               # -1 after 1: the cached plan from the start
            res, x = s.solve_amg(tolerance=TOL, engine=engine)
            assert res.error_code == 0 and res.converged and not res.breakdown, engine
            assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, engine
            assert gpu.csr_has_tiled_plan(s.A) == (engine != 0)
            iters[engine] = res.iterations
        print("poisson2d(64) engines", iters, "restatement", it_ref)
        assert abs(iters[0] - iters[1]) <= 3 and iters[1] == iters[-1], iters
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ stop rules
def test_max_iterations_stops_there_and_steps_after_done_change_nothing(gpu, systems):
    s, _ = systems["poisson2d(32)"]
    full, x_full = s.solve_amg(tolerance=TOL, engine=0)
    assert full.converged and full.iterations >= 3
    for k in (1, 2):
        res, _ = s.solve_amg(tolerance=TOL, engine=0, max_iterations=k)
        assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
    res, x = s.solve_amg(max_iterations=0, x0=np.full(s.n, 0.5, np.float32))
    assert (res.error_code, res.iterations, res.converged) == (0, 0, 0) and np.all(x == np.float32(0.5))
    # stopped by max_iterations at the reported count, and one past it: no step past `done` moved x
    for extra in (0, 1):
        res_k, x_k = s.solve_amg(tolerance=TOL, engine=0, max_iterations=full.iterations + extra)
        assert res_k.iterations == full.iterations and res_k.converged
        assert np.array_equal(bits(x_k), bits(x_full))


def test_zero_b_writes_zeros(gpu):
    s = AMGSystem(gpu, *spd.poisson2d(16), b=np.zeros(256, np.float32))
    try:
        res, x = s.solve_amg(x0=np.full(s.n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(s.n, np.float32))
    finally:
        s.close()


def test_good_initial_guess_returns_at_once_and_leaves_x_alone(gpu, systems):
    s, _ = systems["poisson2d(32)"]
    res, x_solved = s.solve_amg(tolerance=1e-5)
    assert res.converged and res.iterations > 0
    res2, x2 = s.solve_amg(x0=x_solved, tolerance=1e-3)
    assert (res2.error_code, res2.converged, res2.iterations, res2.breakdown) == (0, 1, 0, 0)
    assert np.array_equal(bits(x2), bits(x_solved)) and res2.relative_residual <= 1e-3


def test_a_cycle_that_is_not_positive_definite_breaks_down_or_converges(gpu):
    """omega = 1.9 on the 5-point Laplacian: omega rho(D^-1 A) > 2, so the symmetric cycle is indefinite"""
    s = AMGSystem(gpu, *spd.poisson2d(16), amg=gpu.AMGConfig(jacobi_weight=1.9))
    try:
        x0 = np.full(s.n, 0.25, np.float32)
        res, x = s.solve_amg(x0=x0, tolerance=TOL, engine=0, max_iterations=200)
        print("omega = 1.9:", res.iterations, res.converged, res.breakdown, res.relative_residual)
        assert res.error_code == 0 and np.isfinite(x).all() and np.isfinite(res.relative_residual)
        assert res.breakdown == 1 or res.converged == 1
        if res.breakdown:
            assert res.converged == 0
            # x is the last good iterate: the same solve stopped at that count ends on the same bits
            res_k, x_k = s.solve_amg(x0=x0, tolerance=TOL, engine=0, max_iterations=res.iterations)
            if res_k.breakdown == 0:
                assert np.array_equal(bits(x_k), bits(x))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ rejections
def test_rejections_leave_x_untouched(gpu, systems):
    E = gpu.SpMVError
    s, _ = systems["poisson2d(32)"]
    other, _ = systems["poisson3d(12)"]
    x0 = np.full(s.n, 0.25, np.float32)
    res, x = s.solve_amg(x0=x0, H=None)
    assert res.error_code == E.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))
    res, x = s.solve_amg(x0=x0, H=other.H)
    assert res.error_code == E.INVALID_DIMENSION and np.array_equal(bits(x), bits(x0))
    for pre, post in ((1, 0), (1, 2), (2, 1)):
        res_h, lopsided = gpu.amg_setup(s.A, gpu.AMGConfig(pre_sweeps=pre, post_sweeps=post))
        assert res_h.error_code == 0
        res, x = s.solve_amg(x0=x0, H=lopsided)
        assert res.error_code == E.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0)), (pre, post)
        gpu.amg_destroy(lopsided)
    # cg_solve keeps rejecting a preconditioner value it does not know
    res, x = s.cg(x0=x0, preconditioner=2)
    assert res.error_code == E.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_amg_smoke(gpu, tmp_path):
    """tests/cpp/amg_smoke.cpp through spmv/amg.h, spmv/cg.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "amg_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "amg_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
