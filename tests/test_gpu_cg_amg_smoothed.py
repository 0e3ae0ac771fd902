"""cg_solve_amg (include/spmv/cg.h) preconditioned by one V-cycle of a smoothed-aggregation hierarchy
(amg_setup_smoothed, include/spmv/amg.h).

Checked against the numpy restatement of the documented iteration (test_gpu_cg_ic.py's restate_ic with z from
amg_smoothed_cases' fp32 V-cycle on the levels read back): the device's iteration count equals the restatement's
(one step of slack was allowed for the other order of the row sums; the first run on an MI355X showed equality, 10 / 11
/ 11 / 10 on poisson2d(32) / (48) / (64) / poisson3d(12) against 21 / 23 / 32 / 14 on the plain hierarchies, so
equality is what is asserted), the restatement's smoothed count is strictly below its count on the plain hierarchy of
the same matrix, and the result passes test_gpu_cg_amg.py's residual check.  The steps enqueued
past convergence, every kernel of which reads `done` first, leave x untouched."""
import importlib
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import amg_cases as ac
import amg_smoothed_cases as sc
import test_gpu_bicgstab as base
from conftest import ROOT
from test_gpu_amg_smoothed import view_arrays
from test_gpu_bicgstab import bits, true_residual
from test_gpu_cg_ic import restate_ic

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
TOL = 1e-6

MATRICES = {
    "poisson2d(32)": lambda: spd.poisson2d(32),
    "poisson2d(48)": lambda: spd.poisson2d(48),
    "poisson2d(64)": lambda: spd.poisson2d(64),
    "poisson3d(12)": lambda: spd.poisson3d(12),
}


class SmoothedSystem(base.System):
    """base.System plus the smoothed hierarchy of its matrix, and the levels read back for the restatement"""

    def __init__(self, gpu, n, rp, ci, va, seed=1, amg=None, smoothing=None):
        super().__init__(gpu, n, rp, ci, va, seed=seed)
        self.amg = amg if amg is not None else gpu.AMGConfig()
        self.res, self.H = gpu.amg_setup_smoothed(self.A, self.amg, smoothing)
        assert self.res.error_code == 0 and self.H is not None and gpu.amg_is_smoothed(self.H) == 1
        self.levels = []
        for l in range(self.res.levels):
            m, lrp, lci, lva, agg = gpu.amg_level_arrays(self.H, l)
            level = dict(n=m, rp=lrp, ci=lci, va=lva, agg=agg, count=gpu.amg_level(self.H, l)[3])
            if l + 1 < self.res.levels:
                _, p_view, pt_view = gpu.amg_level_transfer(self.H, l)
                level["P"], level["PT"] = view_arrays(gpu, p_view), view_arrays(gpu, pt_view)
            self.levels.append(level)

    def solve_amg(self, x0=None, **cfg):
        solver = lambda A, d_b, d_x, config: self.gpu.cg_solve_amg(A, self.H, d_b, d_x, config)
        return self._run(solver, self.gpu.CGConfig(**cfg), x0)

    def precondition(self, u):
        c = self.amg
        return sc.vcycle(self.levels, u, c.jacobi_weight, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps, np.float32)

    def close(self):
        self.gpu.amg_destroy(self.H)
        super().close()


def plain_restatement(gpu, s):
    """restate_ic with the fp32 V-cycle of the plain hierarchy of s's matrix (amg_cases.hierarchy, on the host)"""
    levels = ac.hierarchy(gpu, s.n, s.rp, s.ci, s.va)
    c = s.amg
    cycle = lambda u: ac.vcycle(levels, u, c.jacobi_weight, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps, np.float32)
    plain = SimpleNamespace(n=s.n, rp=s.rp, ci=s.ci, va=s.va, b=s.b, precondition=cycle)
    return restate_ic(plain, np.zeros(s.n), TOL)


@pytest.fixture(scope="module")
def systems(gpu):
    """the four Poisson systems with their smoothed hierarchies and both restatements' answers, computed once"""
    built = {}
    for name, make in MATRICES.items():
        s = SmoothedSystem(gpu, *make())
        built[name] = (s, restate_ic(s, np.zeros(s.n), TOL), plain_restatement(gpu, s))
    yield built
    for s, _, _ in built.values():
        s.close()


@pytest.mark.parametrize("name", list(MATRICES))
def test_iterations_follow_the_restatement_and_beat_the_plain_hierarchy(gpu, systems, name):
    s, (x_ref, it_ref, conv_ref, brk_ref, rel_ref), (_, it_plain, conv_plain, _, _) = systems[name]
    assert conv_ref and not brk_ref and conv_plain
    res, x = s.solve_amg(tolerance=TOL, engine=0)
    what = (name, res.iterations, it_ref, it_plain, res.relative_residual, rel_ref)
    print("cg_solve_amg, smoothed: iterations, restatement's, the plain restatement's", what,
          "levels", [lv["n"] for lv in s.levels], "operator complexity %.3f" % s.res.operator_complexity)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    assert res.converged == 1 and res.breakdown == 0, what
    assert res.iterations == it_ref, what
    assert it_ref < it_plain, what
    bound = max(4 * TOL, 2 * true_residual(s.rp, s.ci, s.va, s.b, x_ref))
    assert true_residual(s.rp, s.ci, s.va, s.b, x) <= bound, what
    # two solves, the same bits
    res2, x2 = s.solve_amg(tolerance=TOL, engine=0)
    assert (res2.iterations, res2.relative_residual) == (res.iterations, res.relative_residual)
    assert np.array_equal(bits(x2), bits(x))


def test_steps_after_done_change_nothing(gpu, systems):
    """stopped by max_iterations at the reported count, and with steps to spare: the cycles enqueued past `done`,
    smoothed transfers included, moved nothing"""
    s, _, _ = systems["poisson2d(32)"]
    full, x_full = s.solve_amg(tolerance=TOL, engine=0)
    assert full.converged and full.iterations >= 3
    for extra in (0, 1, 7):
        res_k, x_k = s.solve_amg(tolerance=TOL, engine=0, max_iterations=full.iterations + extra)
        assert res_k.iterations == full.iterations and res_k.converged
        assert np.array_equal(bits(x_k), bits(x_full))
    x0 = np.full(s.n, 0.5, np.float32)
    res, x = s.solve_amg(max_iterations=0, x0=x0)
    assert (res.error_code, res.iterations, res.converged) == (0, 0, 0) and np.all(x == np.float32(0.5))


def test_engines_agree_on_a_tiled_eligible_matrix(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", base.TILED_SMALL)          # lets the tiled engine take a small matrix
    s = SmoothedSystem(gpu, *spd.poisson2d(64))
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
        print("poisson2d(64), smoothed: engines", iters, "restatement", it_ref)
        assert abs(iters[0] - iters[1]) <= 3 and iters[1] == iters[-1], iters
    finally:
        s.close()


def test_the_symmetric_cycle_rule_still_holds(gpu):
    """pre_sweeps != post_sweeps: the hierarchy is built and applies, cg_solve_amg refuses it and leaves x alone"""
    s = SmoothedSystem(gpu, *spd.poisson2d(16), amg=gpu.AMGConfig(post_sweeps=2))
    try:
        x0 = np.full(s.n, 0.25, np.float32)
        res, x = s.solve_amg(x0=x0, tolerance=TOL, engine=0)
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))
        d_z = gpu.CudaBuffer(s.n)
        assert gpu.amg_apply(s.H, s.d_b, d_z) == 0 and np.isfinite(d_z.copyToHost(s.n)).all()
        d_z.release()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ C++ caller
def test_cpp_amg_smoothed_smoke(gpu, tmp_path):
    """tests/cpp/amg_smoothed_smoke.cpp through spmv/amg.h, spmv/cg.h and CudaBuffer, compiled here with build()'s g++
    line."""
    exe = str(tmp_path / "amg_smoothed_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "amg_smoothed_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
