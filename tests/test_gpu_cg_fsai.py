"""cg_solve_fsai (include/spmv/cg.h) on the device, preconditioned by fsai_csr's G and its device transpose.

On poisson2d(16), poisson2d(24) and poisson3d(8) with b uniform in (-1, 1) from default_rng(1), x0 = 0 and tolerance
1e-6: convergence, the true residual, reproducibility, and the iteration counts against Jacobi that are the reason the
preconditioner exists, on A's own pattern and on the pattern of A*A from spgemm_csr; the rejections of G / GT with d_x
unchanged; ||b|| = 0 and a converged x0; a G with a negated row; and that the solve leaves the promotion count and the
tiled plan of A, G and GT alone.

The fp64 restatement of the iteration gave, as Jacobi / FSAI on tril(A) / FSAI on tril(A*A): poisson2d(16) 44 / 24 /
17, poisson2d(24) 64 / 35 / 27, poisson3d(8) 27 / 15 / 11."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import test_gpu_bicgstab as base
from conftest import ROOT
from test_gpu_bicgstab import bits, true_residual

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
JACOBI = 1
TOL = 1e-6

MATRICES = {
    "poisson2d(16)": lambda: spd.poisson2d(16),
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
}


class FSAISystem(base.System):
    """base.System plus G = fsai_csr(A, S) and GT = csr_transpose_gpu(G) on the device; squared: S = spgemm_csr(A, A)"""

    def __init__(self, gpu, n, rp, ci, va, squared=False, b=None):
        super().__init__(gpu, n, rp, ci, va, b=b)
        self.S = None
        if squared:
            self.S = gpu.csr_create(1, 1, 0)
            assert gpu.spgemm_csr(self.S, self.A, self.A).error_code == 0
        self.G, self.GT = gpu.csr_create(1, 1, 0), gpu.csr_create(1, 1, 0)
        self.fsai = gpu.fsai_csr(self.G, self.A, self.S)
        assert self.fsai.error_code == 0 and self.fsai.bad_row == -1
        assert gpu.csr_transpose_gpu(self.GT, self.G) == 0

    def solve_fsai(self, x0=None, G=None, GT=None, **cfg):
        solver = lambda A, d_b, d_x, config: self.gpu.cg_solve_fsai(A, self.G if G is None else G,
                                                                    self.GT if GT is None else GT, d_b, d_x, config)
        return self._run(solver, self.gpu.CGConfig(**cfg), x0)

    def close(self):
        for M in (self.S, self.G, self.GT):
            self.gpu.csr_destroy(M)
        super().close()


@pytest.fixture(scope="module")
def systems(gpu):
    """per matrix: the system on tril(A), the system on tril(A*A), and the Jacobi iteration count, computed once"""
    built = {}
    for name, make in MATRICES.items():
        own = FSAISystem(gpu, *make())
        squared = FSAISystem(gpu, *make(), squared=True)
        jacobi, _ = own.cg(tolerance=TOL, preconditioner=JACOBI, engine=0)
        assert jacobi.error_code == 0 and jacobi.converged
        built[name] = (own, squared, jacobi.iterations)
    yield built
    for own, squared, _ in built.values():
        own.close()
        squared.close()


@pytest.mark.parametrize("name", list(MATRICES))
def test_converges_reproducibly_in_fewer_iterations_than_jacobi(systems, name):
    own, squared, it_jacobi = systems[name]
    counts = {}
    for label, s in (("tril(A)", own), ("tril(A*A)", squared)):
        res, x = s.solve_fsai(tolerance=TOL, engine=0)
        assert res.error_code == 0 and res.converged and not res.breakdown, (name, label)
        assert res.relative_residual <= TOL and res.elapsed_ms > 0, (name, label)
        residual = true_residual(s.rp, s.ci, s.va, s.b, x)
        again, x_again = s.solve_fsai(tolerance=TOL, engine=0)
        counts[label] = res.iterations
        print(f"{name} {label}: Jacobi {it_jacobi}, FSAI {res.iterations} iterations, true residual {residual:.3e}, "
              f"G nnz {s.fsai.nnz}, longest row {s.fsai.max_row}")
        assert residual <= 1e-5, (name, label)
        assert again.iterations == res.iterations and np.array_equal(bits(x_again), bits(x)), (name, label)
        assert bits(np.float32(again.relative_residual)) == bits(np.float32(res.relative_residual)), (name, label)
    assert squared.fsai.nnz > own.fsai.nnz and squared.fsai.max_row > own.fsai.max_row
    assert 3 * counts["tril(A)"] <= 2 * it_jacobi, (name, counts, it_jacobi)
    assert 2 * counts["tril(A*A)"] <= it_jacobi, (name, counts, it_jacobi)


def test_both_engines_agree_on_the_outcome(systems):
    own, _, _ = systems["poisson2d(24)"]
    direct, x0 = own.solve_fsai(tolerance=TOL, engine=0)
    auto, x1 = own.solve_fsai(tolerance=TOL, engine=-1)          # too small for the tiled engine: the same kernels
    assert (auto.error_code, auto.iterations) == (0, direct.iterations) and np.array_equal(bits(x0), bits(x1))
    # config.preconditioner is not read
    res, x2 = own.solve_fsai(tolerance=TOL, engine=0, preconditioner=7)
    assert (res.error_code, res.iterations) == (0, direct.iterations) and np.array_equal(bits(x0), bits(x2))


def test_rejections_leave_x_unchanged(gpu, systems):
    E = gpu.SpMVError
    own, _, _ = systems["poisson2d(16)"]
    other, _, _ = systems["poisson3d(8)"]
    n = own.n
    wide = gpu.csr_wrap_device(n, n + 1, own.G.contents.nnz, own.G.contents.d_row_ptrs, own.G.contents.d_col_indices,
                               own.G.contents.d_values)
    no_values = gpu.csr_wrap_device(n, n, own.G.contents.nnz, own.G.contents.d_row_ptrs, own.G.contents.d_col_indices,
                                    None)
    no_rows = gpu.csr_wrap_device(n, n, own.G.contents.nnz, None, own.G.contents.d_col_indices,
                                  own.G.contents.d_values)
    host_only = gpu.csr_from_arrays(n, n, np.arange(n + 1), np.arange(n), np.ones(n, np.float32))
    x0 = np.full(n, -77.0, np.float32)

    def refused(code, G=None, GT=None, **cfg):
        own.d_x.copyFromHost(x0, n)
        res = gpu.cg_solve_fsai(own.A, own.G if G is None else G, own.GT if GT is None else GT, own.d_b, own.d_x,
                                gpu.CGConfig(**cfg) if cfg else None)
        assert res.error_code == code and (own.d_x.copyToHost(n) == -77.0).all(), (code, G, GT, cfg)

    own.d_x.copyFromHost(x0, n)
    for G, GT in ((None, own.GT), (own.G, None)):
        res = gpu.cg_solve_fsai(own.A, G, GT, own.d_b, own.d_x, None)
        assert res.error_code == E.INVALID_ARGUMENT and (own.d_x.copyToHost(n) == -77.0).all()
    refused(E.INVALID_DIMENSION, G=wide)
    refused(E.INVALID_DIMENSION, GT=wide)
    refused(E.INVALID_DIMENSION, G=other.G)                 # another size than A
    refused(E.INVALID_DIMENSION, GT=other.GT)
    for M in (no_values, no_rows, host_only):
        refused(E.INVALID_FORMAT, G=M)
        refused(E.INVALID_FORMAT, GT=M)
    refused(E.INVALID_ARGUMENT, tolerance=-1.0)             # cg_solve's own checks come first
    refused(E.INVALID_ARGUMENT, G=wide, max_iterations=-1)
    refused(E.INVALID_ARGUMENT, engine=2)
    for M in (wide, no_values, no_rows, host_only):
        gpu.csr_destroy(M)


def test_zero_b_and_a_converged_start(gpu, systems):
    own, _, _ = systems["poisson2d(16)"]
    n = own.n
    zero = FSAISystem(gpu, own.n, own.rp, own.ci, own.va, b=np.zeros(n, np.float32))
    res, x = zero.solve_fsai(x0=np.full(n, 3.0, np.float32), tolerance=TOL)
    assert (res.error_code, res.converged, res.iterations, res.relative_residual) == (0, 1, 0, 0.0)
    assert (x == 0.0).all()
    zero.close()
    first, x = own.solve_fsai(tolerance=TOL, engine=0)
    assert first.converged
    res, x_again = own.solve_fsai(x0=x, tolerance=1e-5, engine=0)
    assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
    assert np.array_equal(bits(x_again), bits(x))
    res, x_cap = own.solve_fsai(tolerance=TOL, max_iterations=5, engine=0)          # the cap, not a hang
    assert (res.error_code, res.converged, res.iterations) == (0, 0, 5) and np.isfinite(x_cap).all()


def test_a_negated_row_of_g_ends_in_a_breakdown_or_a_normal_exit(gpu, systems):
    """GT stays the transpose of the true G, so M^-1 = GT G' is no longer symmetric positive definite"""
    own, _, _ = systems["poisson3d(8)"]
    n = own.n
    assert gpu.csr_from_gpu(own.G) == 0
    g_rp, g_ci, g = gpu.csr_host_arrays(own.G)
    for row in (0, n // 2):
        changed = g.copy()
        changed[g_rp[row]:g_rp[row + 1]] *= -1.0
        G2 = gpu.csr_from_arrays(n, n, g_rp, g_ci, changed)
        assert gpu.csr_to_gpu(G2) == 0
        res, x = own.solve_fsai(G=G2, tolerance=TOL, max_iterations=60, engine=0)
        print(f"negated row {row}: iterations {res.iterations}, converged {res.converged}, breakdown {res.breakdown}")
        assert res.error_code == 0 and res.iterations <= 60 and np.isfinite(x).all()
        assert res.breakdown or res.converged or res.iterations == 60
        gpu.csr_destroy(G2)


def test_the_solve_leaves_promotion_and_the_tiled_plans_alone(gpu):
    """test_gpu_cg.test_auto_engine_builds_and_caches_a_plan_and_leaves_promotion_alone for the FSAI loop: the two
    SpMVs with G and GT are direct launches, so neither matrix gets a plan or a promotion count from the solves, and
    VECTOR_CSR calls promote afterwards exactly as on a fresh matrix"""
    n, rp, ci, va = spd.poisson3d(64)
    s = FSAISystem(gpu, n, rp, ci, va)
    saved = gpu.get_tiled_promotion()
    try:
        gpu.set_tiled_promotion(2)
        for M in (s.A, s.G, s.GT):
            assert gpu.csr_tiled_info(M) is None
        for _ in range(3):
            res, _ = s.solve_fsai(tolerance=TOL, max_iterations=6, engine=0)
            assert (res.error_code, res.iterations) == (0, 6)
            for M in (s.A, s.G, s.GT):
                assert gpu.csr_tiled_info(M) is None and not gpu.csr_has_tiled_plan(M)
        d_y = gpu.CudaBuffer(n)
        for M in (s.A, s.G, s.GT):
            eligible = gpu.tiled_shape(n, n, int(M.contents.nnz))[0]
            for call in range(3):
                assert gpu.spmv_csr(M, s.d_b, d_y, gpu.SpMVConfig(1), n).error_code == 0
                assert gpu.csr_has_tiled_plan(M) == (eligible and call >= 2), call
        d_y.release()
    finally:
        gpu.set_tiled_promotion(saved)
        s.close()


def test_cpp_fsai_smoke(gpu, tmp_path):
    """tests/cpp/fsai_smoke.cpp through spmv/fsai.h, spmv/spgemm.h, spmv/cg.h and CudaBuffer, compiled here with
    build()'s g++ line."""
    exe = str(tmp_path / "fsai_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "fsai_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
