"""cg_solve_multi (include/spmv/cg.h) on the device.

The contract is bitwise: column j of the batched solve is cg_solve(engine = 0) on that column alone.  So the reference
in every comparison is cg_solve itself, and x, iterations, converged, breakdown, error_code and the bits of
relative_residual are compared at zero tolerance, whatever the other columns do.  On top of that: the exact
two-eigenvalue systems past the grid caps (tests/exact_data.py) pin column 0 to the CPU prover's bits, the layouts
(leading dimensions, views 4 bytes past a 16-byte boundary, poisoned padding), columns that finish at different times,
per-column breakdown, the second window of eight columns, reproducibility, isolation from A's caches, the device-side
rejections and a C++ caller."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import exact_data as ed
from array_views import SENTINEL, View
from conftest import ROOT

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
assert_bits = importlib.import_module("test_gpu_lane_sweep").assert_bits

NONE, JACOBI = 0, 1
POISON = SENTINEL.view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Device:
    """A matrix on the device, cg_solve on one column as the reference and cg_solve_multi in any layout."""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n, self.rp = gpu, n, rp
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self.d_b, self.d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        self._single = {}

    def single(self, b, x0, key=None, **cfg):
        """(result, x) of cg_solve(engine = 0) on one column; kept under `key` when one is given."""
        if key is not None and key in self._single:
            return self._single[key]
        self.d_b.copyFromHost(np.asarray(b, np.float32), self.n)
        self.d_x.copyFromHost(np.asarray(x0, np.float32), self.n)
        res = self.gpu.cg_solve(self.A, self.d_b, self.d_x, self.gpu.CGConfig(engine=0, **cfg))
        out = (res, self.d_x.copyToHost(self.n))
        if key is not None:
            self._single[key] = out
        return out

    def multi(self, B, X0, ldb=None, ldx=None, offset=0, engine=0, **cfg):
        """(results, X) of cg_solve_multi on the n x k arrays B and X0, stored with the given leading dimensions in
        views `offset` floats past a 16-byte boundary.  X's padding columns and both views' surroundings are poison:
        asserts that they, and B, come back bit for bit."""
        n, k = B.shape
        ldb, ldx = ldb or k, ldx or k
        hb = np.full((n, ldb), POISON, np.float32)
        hx = np.full((n, ldx), POISON, np.float32)
        hb[:, :k], hx[:, :k] = B, X0
        vb = View(self.gpu, hb.ravel(), offset, SENTINEL)
        vx = View(self.gpu, hx.ravel(), offset, SENTINEL)
        try:
            results = self.gpu.cg_solve_multi(self.A, vb.ptr, vx.ptr, k, ldb, ldx,
                                              self.gpu.CGConfig(engine=engine, **cfg))
            got = vx.download().reshape(n, ldx)
            vb.check_guards("B")
            vx.check_guards("X")
            assert np.array_equal(bits(vb.download()), bits(hb.ravel())), "B was written"
            assert np.array_equal(bits(got[:, k:]), bits(hx[:, k:])), "X's padding columns were written"
            return results, got[:, :k].copy()
        finally:
            vb.release()
            vx.release()

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def assert_column(rp, res, x, ref, x_ref, what):
    """One column of the batch against its own cg_solve run, to the bit."""
    got = (res.error_code, res.iterations, res.converged, res.breakdown)
    want = (ref.error_code, ref.iterations, ref.converged, ref.breakdown)
    assert got == want, (what, got, want)
    rel, rel_ref = np.float32(res.relative_residual), np.float32(ref.relative_residual)
    assert rel.view(np.uint32) == rel_ref.view(np.uint32), (what, rel, rel_ref)
    assert_bits(rp, x, x_ref, what)


def assert_parity(dev, B, X0, what, keys=None, layout=None, **cfg):
    """cg_solve_multi on (B, X0) against cg_solve column by column; returns (results, X)."""
    results, X = dev.multi(B, X0, **dict(layout or {}, **cfg))
    assert len(results) == B.shape[1]
    assert len({r.elapsed_ms for r in results}) == 1
    for j in range(B.shape[1]):
        ref, x_ref = dev.single(B[:, j], X0[:, j], key=None if keys is None else keys[j], **cfg)
        assert_column(dev.rp, results[j], X[:, j], ref, x_ref, what + ("column", j))
    return results, X


def columns(n, b, k, seed=7):
    """B (n x k): the system's own b, then seeded uniform columns (column j the same whatever k)."""
    B = np.empty((n, k), np.float32)
    B[:, 0] = b
    for j in range(1, k):
        B[:, j] = np.random.default_rng([seed, j]).uniform(-64.0, 64.0, n).astype(np.float32)
    return B


# ------------------------------------------------------------------------------------------ 1. every lane count
ALL_K = (1, 2, 3, 4, 5, 8, 9, 16, 32)
FULL_K_NAMES = ("L1_low", "L16_top")


@pytest.mark.parametrize("precond", [NONE, JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_column_parity_at_every_lane_count(gpu, name, precond):
    """cgm_init_kernel<L, 4, W>, cgm_spmv_dot<L, W, NW> in all four (W, NW) forms on two names and in (4, 1), (8, 1),
    (8, 2) on the rest, cgm_update_kernel / cgm_direction_kernel<4 and 8>: 1201 / 1202 rows, five workgroups."""
    L, n, rp, ci, va, _, b = ed.solver_system(name, symmetric=True)
    dev = Device(gpu, n, rp, ci, va)
    try:
        iterations = set()
        for k in (ALL_K if name in FULL_K_NAMES else (3, 8, 9)):
            B = columns(n, b, k)
            cfg = dict(tolerance=1e-6, max_iterations=60, preconditioner=precond)
            results, _ = assert_parity(dev, B, np.zeros_like(B), (name, L, precond, k), keys=list(range(k)), **cfg)
            assert all(r.error_code == 0 and r.iterations > 0 for r in results)
            iterations |= {r.iterations for r in results}
        print(name, "iterations seen", sorted(iterations))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 2. layouts
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("ldb,ldx", [(5, 5), (8, 8), (7, 6), (5, 12)])
@pytest.mark.parametrize("name", ["L4_top", "L16_low"])
def test_leading_dimensions_and_alignment(gpu, name, ldb, ldx, offset):
    """k = 5: dwordx4 slices of X only at (8, 8) / (5, 12) with offset 0 and only for columns 0..3; guarded scalar loads
    everywhere else.  Device.multi asserts the poison in X's padding columns, around both arrays, and B itself."""
    L, n, rp, ci, va, x_star, b = ed.solver_system(name, symmetric=True)
    dev = Device(gpu, n, rp, ci, va)
    try:
        B = columns(n, b, 5)
        X0 = np.zeros_like(B)
        X0[:, 2] = x_star                                            # a non-zero guess goes through cgm_init_kernel's walk
        for precond in (NONE, JACOBI):
            assert_parity(dev, B, X0, (name, ldb, ldx, offset, precond), keys=[(precond, j) for j in range(5)],
                          layout=dict(ldb=ldb, ldx=ldx, offset=offset), tolerance=1e-6, max_iterations=60,
                          preconditioner=precond)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. finishing apart
def poisson_mode(m, i, j):
    """An eigenvector of poisson2d(m): CG on a multiple of it ends after one step (a few in fp32)."""
    s = np.sin(np.pi * np.arange(1, m + 1) / (m + 1) * i)
    t = np.sin(np.pi * np.arange(1, m + 1) / (m + 1) * j)
    return np.outer(s, t).ravel()


def test_columns_that_finish_at_different_times(gpu):
    """poisson2d(64), k = 6: a zero column (x = 0), a column whose guess already meets the tolerance (0 iterations, x
    untouched), one eigenvector (b = A e up to rounding: a handful of steps), two draws from the span of three and of
    eight eigenvectors (they finish in the teens), one uniform draw that max_iterations = 25 cuts off, and then
    the same batch with room for every column.  A frozen column sits in a window with running ones throughout."""
    m = 64
    n, rp, ci, va = spd.poisson2d(m)
    dev = Device(gpu, n, rp, ci, va)
    try:
        rng = np.random.default_rng(21)
        tol = 1e-4                                                   # two decades above the guess of column 1
        B = np.zeros((n, 6), np.float32)
        X0 = rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32)       # the zero column's guess must be overwritten
        B[:, 1] = rng.uniform(-1.0, 1.0, n)
        solved, x_solved = dev.single(B[:, 1], np.zeros(n), tolerance=1e-6, preconditioner=JACOBI)
        assert solved.converged and solved.iterations > 25
        X0[:, 1] = x_solved
        B[:, 2] = spd.spmv64(rp, ci, va, poisson_mode(m, 3, 5))
        B[:, 3] = sum(w * poisson_mode(m, i, j) for w, (i, j) in zip(rng.uniform(0.5, 2.0, 3), [(1, 1), (7, 2), (20, 33)]))
        B[:, 4] = sum(w * poisson_mode(m, i, i + 3) for w, i in zip(rng.uniform(0.5, 2.0, 8), range(2, 50, 6)))
        B[:, 5] = rng.uniform(-1.0, 1.0, n)
        X0[:, 2:] = 0.0
        for precond in (JACOBI, NONE):
            results, X = assert_parity(dev, B, X0, ("finish", precond, 25), tolerance=tol, max_iterations=25,
                                       preconditioner=precond)
            its = [r.iterations for r in results]
            print("preconditioner", precond, "iterations", its, "converged", [r.converged for r in results])
            assert (its[0], results[0].converged) == (0, 1) and not X[:, 0].any()
            assert (its[1], results[1].converged) == (0, 1) and np.array_equal(bits(X[:, 1]), bits(X0[:, 1]))
            assert 1 <= its[2] <= 5 and results[2].converged
            assert its[2] < its[3] < 25 and its[2] < its[4] < 25 and results[3].converged and results[4].converged
            assert (its[5], results[5].converged, results[5].breakdown) == (25, 0, 0)
            results, _ = assert_parity(dev, B, X0, ("finish", precond, 1000), tolerance=tol, max_iterations=1000,
                                       preconditioner=precond)
            assert all(r.converged for r in results) and results[5].iterations > 25
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 4. breakdown per column
def dense_device(gpu, dense):
    dense = np.asarray(dense, np.float32)
    n = dense.shape[0]
    rows, cols = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return Device(gpu, n, rp, cols.astype(np.int32), dense[rows, cols])


def test_breakdown_is_per_column(gpu):
    """NONE on diag(1, -1, 2, 3): b = e0 converges, b = e1 breaks down at step 0 (p.Ap = -1) with x at its guess, the
    mixed b = e0 + e1 + e2 does what cg_solve does.  JACOBI on a positive diagonal with the indefinite block
    [[1, 2], [2, 1]]: b = e2 converges, b = e0 breaks down at step 1, b = (1, 1, 0, 0) is an eigenvector (3) and
    converges, b = (1, -1, 1, 1) meets the eigenvalue -1 at step 0."""
    eye = np.eye(4, dtype=np.float32)
    cases = [(NONE, np.diag([1.0, -1.0, 2.0, 3.0]), [eye[0], eye[1], eye[0] + eye[1] + eye[2], eye[3]],
              [(1, 0, None), (0, 1, 0), None, (1, 0, None)]),
             (JACOBI, [[1, 2, 0, 0], [2, 1, 0, 0], [0, 0, 2, 0], [0, 0, 0, 4]],
              [eye[2], eye[0], eye[0] + eye[1], np.array([1, -1, 1, 1], np.float32)],
              [(1, 0, 1), (0, 1, 1), (1, 0, 1), (0, 1, 0)])]
    for precond, dense, bs, expect in cases:
        dev = dense_device(gpu, dense)
        try:
            B = np.stack(bs, axis=1).astype(np.float32)
            X0 = np.zeros_like(B)
            if precond == NONE:
                X0[1, 1] = 0.75                                      # r0 = 1.75 e1: still the eigenvalue -1 alone
            results, X = assert_parity(dev, B, X0, ("breakdown", precond), tolerance=1e-6, max_iterations=20,
                                       preconditioner=precond)
            for j, want in enumerate(expect):
                if want is None:
                    continue
                r = results[j]
                assert (r.converged, r.breakdown) == want[:2], (precond, j, r.converged, r.breakdown, r.iterations)
                assert want[2] is None or r.iterations == want[2], (precond, j, r.iterations)
                assert np.all(np.isfinite(X[:, j])) and np.isfinite(r.relative_residual)
            if precond == NONE:                                      # broken down before any update: x is the guess
                assert np.array_equal(bits(X[:, 1]), bits(X0[:, 1]))
        finally:
            dev.close()


# ------------------------------------------------------------------------------------------ 5. past the grid caps
TRIP_CASES = [(ed.VEC_TRIP + 1, 1), (ed.row_trip(1) + 257, 1), (ed.LANE_SIZES[8], 8), (ed.LANE_SIZES[64], 64)]
SCALES = (1.0, 2.0, 0.25)


def assert_scales_are_exact(system):
    """The prover (tests/test_exact_data.py prove_cg) shows every stored quantity of the solve to be a dyadic rational
    that fp32 holds and every dot product exact in fp64.  A power-of-two factor on b moves the exponents of all of
    them by the same amount and no mantissa, alpha and beta not at all, so the scaled solve is exact as long as no
    exponent leaves the normal range: everything the solve stores is within a factor ||A||_inf^2 of b's entries."""
    rows = np.diff(system["rp"].astype(np.int64))
    norm = float(np.abs(system["va"].astype(np.float64)).max()) * float(rows.max())
    nonzero = np.abs(system["b"][system["b"] != 0]).astype(np.float64)
    for s in SCALES:
        assert np.log2(s) == np.rint(np.log2(s))
        assert nonzero.max() * s * norm * norm < 2.0 ** 100 and nonzero.min() * s / (norm * norm) > 2.0 ** -100
        for v in (system["b"], system["x1"], system["x2"]):
            scaled = (v * np.float32(s)).astype(np.float32)
            assert np.array_equal(bits(scaled / np.float32(s)), bits(v))


@pytest.mark.parametrize("precond", [NONE, JACOBI], ids=["none", "jacobi"])
@pytest.mark.parametrize("n,L", TRIP_CASES, ids=["n%d_L%d" % c for c in TRIP_CASES])
def test_exact_two_steps_past_the_grid_caps(gpu, n, L, precond):
    """k = 3 with B = (b, 2 b, b / 4) on the two-eigenvalue systems: the element-wise kernels take a second trip of
    one row (V + 1), the row kernels a second trip (R_1 + 257, R_8 + 33, R_64 + 5).  All three scales fit (asserted);
    column 0 is the prover's x2 / x1 to the bit, the others are its multiples, all three are cg_solve's."""
    system = ed.two_eig_system("cg", n, L, scaled=precond == JACOBI)
    assert_scales_are_exact(system)
    dev = Device(gpu, n, system["rp"], system["ci"], system["va"])
    try:
        B = np.stack([system["b"] * np.float32(s) for s in SCALES], axis=1).astype(np.float32)
        X0 = np.zeros_like(B)
        what = ("two steps", n, L, precond)
        results, X = assert_parity(dev, B, X0, what, tolerance=1e-6, max_iterations=50, preconditioner=precond)
        for j, s in enumerate(SCALES):
            r = results[j]
            assert (r.error_code, r.iterations, r.converged, r.breakdown) == (0, 2, 1, 0), (what, j, r.iterations)
            assert r.relative_residual == 0.0, (what, j, r.relative_residual)
            assert_bits(system["rp"], X[:, j], system["x2"] * np.float32(s), what + (j,))
        what = ("one step", n, L, precond)
        results, X = assert_parity(dev, B, X0, what, tolerance=0.0, max_iterations=1, preconditioner=precond)
        for j, s in enumerate(SCALES):
            r = results[j]
            assert (r.error_code, r.iterations, r.converged, r.breakdown) == (0, 1, 0, 0), (what, j, r.iterations)
            got, want = np.float32(r.relative_residual), system["rel1"]
            ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
            print(what, "column", j, "relative_residual", got, "predicted", want, "ulps", ulps)
            assert ulps <= 1, (what, j, got, want)
            assert_bits(system["rp"], X[:, j], system["x1"] * np.float32(s), what + (j,))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. the second window
@pytest.mark.parametrize("k", [9, 12, 17])
def test_only_the_first_column_of_the_second_window_runs(gpu, k):
    """Column 8 is the only non-zero column: window 0 is frozen from the start and never walked."""
    L, n, rp, ci, va, x_star, b = ed.solver_system("L4_top", symmetric=True)
    dev = Device(gpu, n, rp, ci, va)
    try:
        B = np.zeros((n, k), np.float32)
        B[:, 8] = b
        X0 = np.tile(x_star[:, None], (1, k)).astype(np.float32)
        results, X = assert_parity(dev, B, X0, ("window", k), tolerance=1e-6, max_iterations=60, preconditioner=JACOBI)
        assert results[8].iterations > 0 and results[8].converged
        for j in range(k):
            if j != 8:
                assert (results[j].iterations, results[j].converged) == (0, 1) and not X[:, j].any()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 7. reproducibility, isolation
def test_two_runs_and_a_column_permutation_give_the_same_bits(gpu):
    n, rp, ci, va = spd.random_spd(20_000, 7, seed=11)
    dev = Device(gpu, n, rp, ci, va)
    try:
        k = 11
        rng = np.random.default_rng(3)
        B = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
        B[:, 4] = 0.0
        X0 = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
        cfg = dict(tolerance=1e-6, max_iterations=200, preconditioner=JACOBI)
        fields = lambda rs: [(r.error_code, r.iterations, r.converged, r.breakdown,
                              int(np.float32(r.relative_residual).view(np.uint32))) for r in rs]
        r1, x1 = dev.multi(B, X0, **cfg)
        r2, x2 = dev.multi(B, X0, **cfg)
        assert fields(r1) == fields(r2) and np.array_equal(bits(x1), bits(x2))
        assert all(r.converged for r in r1) and len({r.iterations for r in r1}) > 1
        perm = rng.permutation(k)
        r3, x3 = dev.multi(B[:, perm], X0[:, perm], ldb=13, ldx=16, **cfg)
        assert fields(r3) == [fields(r1)[j] for j in perm]
        assert np.array_equal(bits(x3), bits(x1[:, perm]))
    finally:
        dev.close()


def test_the_call_leaves_promotion_and_the_tiled_plan_alone(gpu):
    """test_gpu_cg.test_auto_engine_builds_and_caches_a_plan_and_leaves_promotion_alone for the batched call: on a
    tiled-eligible matrix neither engine value builds a plan, and VECTOR_CSR calls promote afterwards exactly as on a
    fresh matrix."""
    n, rp, ci, va = spd.poisson3d(64)
    assert gpu.tiled_shape(n, n, ci.size)[0]
    dev = Device(gpu, n, rp, ci, va)
    saved = gpu.get_tiled_promotion()
    try:
        gpu.set_tiled_promotion(2)
        B = np.random.default_rng(5).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        for engine in (0, -1, 0):
            results, _ = dev.multi(B, np.zeros_like(B), engine=engine, tolerance=1e-6, max_iterations=6)
            assert all((r.error_code, r.iterations) == (0, 6) for r in results)
            assert not gpu.csr_has_tiled_plan(dev.A)
        d_y = gpu.CudaBuffer(n)
        dev.d_b.copyFromHost(B[:, 0].copy(), n)
        for call in range(3):
            assert gpu.spmv_csr(dev.A, dev.d_b, d_y, gpu.SpMVConfig(1), n).error_code == 0
            assert gpu.csr_has_tiled_plan(dev.A) == (call >= 2), call
        d_y.release()
    finally:
        gpu.set_tiled_promotion(saved)
        dev.close()


# ------------------------------------------------------------------------------------------ 8. device-side rejection
def test_bad_diagonal_and_the_tiled_engine_are_rejected_with_x_untouched(gpu):
    rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [4, .5, .5, 3, -2, 5]           # (2, 2) = -2
    dev = Device(gpu, 4, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float32))
    try:
        B = np.ones((4, 3), np.float32)
        X0 = np.arange(12, dtype=np.float32).reshape(4, 3) + 0.5
        E = gpu.SpMVError
        for cfg, code in ((dict(preconditioner=JACOBI), E.INVALID_ARGUMENT),
                          (dict(preconditioner=NONE, engine=1), E.INVALID_ARGUMENT),
                          (dict(preconditioner=JACOBI, engine=1), E.INVALID_ARGUMENT)):
            results, X = dev.multi(B, X0, ldx=4, **cfg)
            assert [r.error_code for r in results] == [code] * 3, cfg
            assert all((r.iterations, r.converged, r.breakdown) == (0, 0, 0) for r in results)
            assert np.array_equal(bits(X), bits(X0)), cfg
        ref, _ = dev.single(B[:, 0], X0[:, 0], preconditioner=JACOBI)
        assert ref.error_code == E.INVALID_ARGUMENT                                  # cg_solve's own verdict
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 9. C++ caller
def test_cpp_cg_multi_smoke(gpu, tmp_path):
    """tests/cpp/cg_multi_smoke.cpp through spmv/cg.h and CudaBuffer, compiled here with test_cpp_cg_smoke's g++ line."""
    exe = str(tmp_path / "cg_multi_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "cg_multi_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
