"""gmres_solve / gmres_solve_lu (include/spmv/gmres.h) on the device.

What GMRES(m) promises here and BiCGSTAB does not is checked first: a restart is bit for bit a new solve from the
current x, the reported residual is the recomputed one (to the fp32 rounding of one SpMV,
gmres_cases.residual_rounding_bound), and it never grows with the step count.  Then the solver is compared with the
numpy restatement of the header (tests/gmres_cases.py) at fixed step counts and on converged solves.

The tolerance of that comparison was measured on the CPU as the spread of the restatement between two SpMV summation
orders (sequential fp32 row sums against fp64 sums rounded once) over gmres_cases.SYSTEMS, NONE and JACOBI,
(restart, k) in (8, 1), (8, 3), (8, 8), (30, 1), (30, 3), (30, 8), (30, 20): the relative residual moves by at most
1.0e-4 of itself (random_63, JACOBI, k = 8, residual 1.9e-4), and the iteration count of solves converged to 1e-5
(restart 8 and 30) by 0.  The device's order is a third one, so the residual is held to 4 x 1.0e-4 = 4e-4 of itself
(SPREAD) plus the rounding bounds of the two recomputed residuals, and the iteration count to 4 x 0 = 0."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import gmres_cases as gc
from conftest import ROOT

pytestmark = pytest.mark.gpu

nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
NONE, JACOBI = gc.NONE, gc.JACOBI
TILED_SMALL = "min_cols=1,min_nnz=1"
SPREAD = 4 * 1.0e-4


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class System:
    """A matrix on the device (csr_from_arrays + csr_to_gpu) with device b and x buffers."""

    def __init__(self, gpu, n, rp, ci, va, seed=1, b=None):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self.b = gc.rhs(n, seed) if b is None else np.asarray(b, np.float32)
        self.d_b = gpu.CudaBuffer(n)
        self.d_x = gpu.CudaBuffer(n)
        self.d_b.copyFromHost(self.b, n)
        self.F = self.d_lu = None

    def solve(self, x0=None, LU=None, **cfg):
        x0 = np.zeros(self.n, np.float32) if x0 is None else np.asarray(x0, np.float32)
        self.d_x.copyFromHost(x0, self.n)
        config = self.gpu.GMRESConfig(**cfg)
        if LU is None:
            res = self.gpu.gmres_solve(self.A, self.d_b, self.d_x, config)
        else:
            res = self.gpu.gmres_solve_lu(self.A, LU, self.d_b, self.d_x, config)
        return res, self.d_x.copyToHost(self.n)

    def factor(self):
        """the ILU(0) factor of ilu0_csr, wrapped over A's structure arrays"""
        gpu = self.gpu
        self.d_lu = gpu.CudaBuffer(self.ci.size)
        res = gpu.ilu0_csr(self.A, self.d_lu)
        assert res.error_code == 0 and res.zero_pivot == -1
        self.F = gpu.csr_wrap_device(self.n, self.n, int(self.ci.size), self.A.contents.d_row_ptrs,
                                     self.A.contents.d_col_indices, self.d_lu.get())
        return self.F

    def true(self, x):
        return gc.true_residual(self.rp, self.ci, self.va, self.b, x)

    def bound(self, x):
        return gc.residual_rounding_bound(self.rp, self.ci, self.va, self.b, x)

    def close(self):
        if self.F is not None:
            self.gpu.csr_destroy(self.F)
            self.d_lu.release()
        self.gpu.csr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def check_honest(s, res, x, tol=None):
    """relative_residual is ||b - A x|| / ||b|| of the returned x: the device's fp32 SpMV and subtraction against
    fp64, within the rounding of one SpMV (any summation order, gmres_cases.residual_rounding_bound) plus the
    rounding of the reported float; converged means that figure passes the tolerance within the same bound"""
    true, bound = s.true(x), s.bound(x)
    print("reported", res.relative_residual, "true", true, "bound", bound)
    assert abs(res.relative_residual - true) <= bound + 2.0 ** -23 * true, (res.relative_residual, true, bound)
    if tol is not None and res.converged:
        assert true <= float(np.float32(tol)) + bound, (true, tol, bound)


@pytest.fixture(scope="module")
def cd64(gpu):
    s = System(gpu, *nonsym.convdiff2d(64, 5.0))
    yield s
    s.close()


# ------------------------------------------------------------------------------------------ 1. restart identity
@pytest.mark.parametrize("engine", [0, 1])
@pytest.mark.parametrize("m", gc.RESTARTS)
def test_a_restart_is_a_new_solve_from_the_current_x(gpu, monkeypatch, m, engine):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)               # lets the tiled engine take a small matrix
    systems = [nonsym.convdiff2d(64, 5.0)] if engine == 0 else [nonsym.convdiff2d(64, 5.0),
                                                                nonsym.random_nonsym(3000, 7, seed=3,
                                                                                     negative_rows=0.25)]
    for n, rp, ci, va in systems:
        s = System(gpu, n, rp, ci, va)
        try:
            for precond in (NONE, JACOBI):
                cfg = dict(tolerance=0.0, restart=m, preconditioner=precond, engine=engine)
                one, x_one = s.solve(max_iterations=2 * m, **cfg)
                first, x_first = s.solve(max_iterations=m, **cfg)
                second, x_second = s.solve(x0=x_first, max_iterations=m, **cfg)
                assert (one.error_code, first.error_code, second.error_code) == (0, 0, 0)
                assert (one.iterations, one.restarts, first.iterations, first.restarts, second.iterations) == \
                    (2 * m, 1, m, 0, m), (n, m, precond)
                assert np.array_equal(bits(x_one), bits(x_second)), (n, m, precond)
                assert bits(one.relative_residual) == bits(second.relative_residual), (n, m, precond)
            assert bool(gpu.csr_has_tiled_plan(s.A)) == (engine == 1)
        finally:
            s.close()


# ------------------------------------------------------------------------------------------ 2. reproducibility
def test_five_runs_give_the_same_bits(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)
    s = System(gpu, *nonsym.random_nonsym(3000, 7, seed=11, negative_rows=0.25))
    try:
        for engine in (0, 1):
            for precond in (NONE, JACOBI):
                runs = [s.solve(tolerance=1e-6, restart=9, engine=engine, preconditioner=precond) for _ in range(5)]
                r0, x0 = runs[0]
                assert r0.error_code == 0 and r0.converged and r0.restarts >= 1, (engine, precond, r0.iterations)
                for r, x in runs[1:]:
                    assert (r.iterations, r.restarts, r.relative_residual) == \
                        (r0.iterations, r0.restarts, r0.relative_residual)
                    assert np.array_equal(bits(x), bits(x0)), (engine, precond)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 3. honest residual
@pytest.mark.parametrize("name", list(gc.SYSTEMS))
def test_the_reported_residual_is_the_recomputed_one(gpu, name):
    s = System(gpu, *gc.SYSTEMS[name]())
    try:
        for precond in (NONE, JACOBI):
            for m in (1, 8, 30):
                for tol, cap in ((1e-5, 1000), (1e-7, 12)):
                    res, x = s.solve(tolerance=tol, max_iterations=cap, restart=m, preconditioner=precond, engine=0)
                    assert res.error_code == 0 and res.breakdown == 0, (name, precond, m)
                    check_honest(s, res, x, tol)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 4. monotone
def test_the_residual_never_grows_with_the_step_count(gpu):
    s = System(gpu, *nonsym.convdiff2d(16, 2.0))
    try:
        for precond in (NONE, JACOBI):
            for m in (8, 30):
                rels, bound = [], 0.0
                for k in range(0, m + 1):
                    res, x = s.solve(tolerance=0.0, max_iterations=k, restart=m, preconditioner=precond, engine=0)
                    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, k, 0, 0)
                    rels.append(float(res.relative_residual))
                    bound = max(bound, s.bound(x))
                # each figure is its true residual to `bound`, and GMRES minimises over growing spaces
                assert all(b <= a + 2 * bound for a, b in zip(rels, rels[1:])), (precond, m, rels)
                assert rels[-1] < 0.5 * rels[0]
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 5. the restatement
@pytest.mark.parametrize("name", list(gc.SYSTEMS))
def test_against_the_restatement(gpu, name):
    """Fixed step counts to SPREAD (module docstring); converged solves on the iteration count, margin 0."""
    n, rp, ci, va = gc.SYSTEMS[name]()
    s = System(gpu, n, rp, ci, va)
    try:
        for precond in (NONE, JACOBI):
            for m, k in ((8, 1), (8, 8), (8, 20), (30, 20)):
                res, x = s.solve(tolerance=0.0, max_iterations=k, restart=m, preconditioner=precond, engine=0)
                x_ref, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, s.b, np.zeros(n), 0.0, k, m, precond)
                what = (name, precond, m, k, res.iterations, it, res.relative_residual, rel)
                print(what)
                assert (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown) == \
                    (0, it, restarts, int(conv), brk), what
                assert abs(res.relative_residual - rel) <= SPREAD * rel + s.bound(x) + s.bound(x_ref), what
            for m in (8, 30):
                res, x = s.solve(tolerance=1e-5, restart=m, preconditioner=precond, engine=0)
                x_ref, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, s.b, np.zeros(n), 1e-5, 1000, m,
                                                                 precond)
                what = (name, precond, m, res.iterations, it, res.restarts, restarts, res.relative_residual, rel)
                print(what)
                assert conv and res.error_code == 0 and res.converged == 1 and res.breakdown == 0, what
                assert (res.iterations, res.restarts) == (it, restarts), what
                assert res.elapsed_ms > 0
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 6. lucky breakdown
def test_lucky_breakdown_is_not_an_error(gpu):
    n = 300
    rng = np.random.default_rng(5)
    d = np.ldexp(np.float32(1.0), rng.integers(-3, 6, n)).astype(np.float32)
    d[rng.random(n) < 0.5] *= -1
    b = np.zeros(n, np.float32)
    b[0] = 32.0
    s = System(gpu, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d, b=b)
    try:
        for precond in (NONE, JACOBI):
            res, x = s.solve(tolerance=1e-6, preconditioner=precond, engine=0)
            assert (res.error_code, res.converged, res.iterations, res.restarts, res.breakdown) == (0, 1, 1, 0, 0)
            want = np.zeros(n, np.float32)
            want[0] = np.float32(32.0) / d[0]
            assert np.array_equal(bits(x), bits(want)) and res.relative_residual == 0.0
    finally:
        s.close()


def test_a_system_smaller_than_the_restart_converges_within_n_steps(gpu):
    rng = np.random.default_rng(8)
    dense = rng.uniform(-1, 1, (5, 5)).astype(np.float32) + 4 * np.eye(5, dtype=np.float32)
    rows, cols = np.nonzero(dense)
    rp = np.zeros(6, np.int32)
    np.cumsum(np.bincount(rows, minlength=5), out=rp[1:])
    s = System(gpu, 5, rp, cols.astype(np.int32), dense[rows, cols])
    try:
        for precond in (NONE, JACOBI):
            res, x = s.solve(tolerance=1e-5, restart=30, preconditioner=precond, engine=0)
            assert res.error_code == 0 and res.converged == 1 and res.breakdown == 0 and res.iterations <= 5, \
                (precond, res.iterations)
            check_honest(s, res, x, 1e-5)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 7. breakdowns
@pytest.mark.parametrize("case", ["2x2", "random_65"])
def test_singular(gpu, case):
    """A zero row and column that b reaches: A v_0 = 0, the rotated column is 0.  No Jacobi diagonal exists."""
    if case == "2x2":
        n, rp, ci, va, at = 2, np.array([0, 1, 1], np.int32), np.array([0], np.int32), np.array([2.0], np.float32), 1
    else:
        n, rp, ci, va = gc.SYSTEMS["random_65"]()
        at = 10
        rows = np.repeat(np.arange(n), np.diff(rp))
        keep = (rows != at) & (ci != at)
        rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
        ci, va = ci[keep], va[keep]
    b = np.zeros(n, np.float32)
    b[at] = 1.0
    x0 = np.zeros(n, np.float32)
    x0[at] = 5.0                                        # the zero column: A x0 = 0
    s = System(gpu, n, rp, ci, va, b=b)
    try:
        res, x = s.solve(x0=x0, preconditioner=NONE, engine=0)
        assert (res.error_code, res.breakdown, res.converged, res.iterations) == (0, gpu.GMRES_SINGULAR, 0, 0)
        assert np.all(np.isfinite(x)) and np.array_equal(bits(x), bits(x0)) and res.relative_residual == 1.0
        ref = gc.restate(n, rp, ci, va, b, x0, 1e-6, 1000, 30, NONE)
        assert (ref[1], ref[3], ref[4]) == (0, False, gc.SINGULAR)
        res, x = s.solve(x0=x0, preconditioner=JACOBI, engine=0)
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT and np.array_equal(bits(x), bits(x0))
    finally:
        s.close()


def test_not_finite_leaves_x_at_the_guess(gpu):
    n, rp, ci, va = gc.SYSTEMS["random_257"]()
    b = gc.rhs(n)
    b[100] = np.inf
    s = System(gpu, n, rp, ci, va, b=b)
    try:
        x0 = np.full(n, 0.25, np.float32)
        for precond in (NONE, JACOBI):
            res, x = s.solve(x0=x0, preconditioner=precond, engine=0)
            assert (res.error_code, res.breakdown, res.converged, res.iterations) == \
                (0, gpu.GMRES_NOT_FINITE, 0, 0), precond
            assert np.array_equal(bits(x), bits(x0))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 8. preconditioners
def test_ilu0_beats_jacobi_beats_nothing_and_an_identity_factor_is_none(gpu):
    n, rp, ci, va = nonsym.convdiff2d(64, 50.0)
    s = System(gpu, n, rp, ci, va)
    eye = gpu.csr_from_arrays(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32),
                              np.ones(n, np.float32))
    assert gpu.csr_to_gpu(eye) == 0
    try:
        F = s.factor()
        lu, x_lu = s.solve(LU=F, tolerance=1e-6, engine=0)
        jac, x_jac = s.solve(tolerance=1e-6, preconditioner=JACOBI, engine=0)
        non, x_non = s.solve(tolerance=1e-6, preconditioner=NONE, engine=0)
        print("steps: ILU(0)", lu.iterations, "JACOBI", jac.iterations, "NONE", non.iterations)
        for res, x in ((lu, x_lu), (jac, x_jac), (non, x_non)):
            assert res.error_code == 0 and res.converged == 1 and res.breakdown == 0
            check_honest(s, res, x, 1e-6)
        assert lu.iterations < jac.iterations <= non.iterations
        # the preconditioner field is not read by gmres_solve_lu
        lu2, x_lu2 = s.solve(LU=F, tolerance=1e-6, engine=0, preconditioner=7)
        assert (lu2.error_code, lu2.iterations) == (0, lu.iterations) and np.array_equal(bits(x_lu2), bits(x_lu))
        # M = I as a factor: NONE's bits
        ident, x_ident = s.solve(LU=eye, tolerance=1e-6, engine=0)
        assert (ident.error_code, ident.iterations, ident.restarts) == (0, non.iterations, non.restarts)
        assert np.array_equal(bits(x_ident), bits(x_non)) and ident.relative_residual == non.relative_residual
    finally:
        gpu.csr_destroy(eye)
        s.close()


@pytest.mark.parametrize("case", ["zero", "nan", "missing", "malformed", "size"])
def test_a_bad_factor_is_rejected_and_x_is_untouched(gpu, case):
    E = gpu.SpMVError
    a_rp, a_ci, a_va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, -3, 2, 1, 1, 5]
    rows, want = 4, E.INVALID_ARGUMENT
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = a_rp, a_ci, [4, .5, .5, -3, 0, 1, 1, 5]
    elif case == "nan":                         # (2,2) = NaN
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [4, .5, .5, -3, np.nan, 5]
    elif case == "missing":                     # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [4, .5, .5, -3, 1, 1]
    elif case == "malformed":                   # a column past the matrix: INVALID_FORMAT from the analysis
        rp, ci, va, want = a_rp, [0, 1, 0, 9, 2, 3, 2, 3], a_va, E.INVALID_FORMAT
    else:                                       # another size
        rows, rp, ci, va, want = 3, [0, 1, 2, 3], [0, 1, 2], [1, 1, 1], E.INVALID_DIMENSION
    A = gpu.csr_from_arrays(4, 4, a_rp, a_ci, np.asarray(a_va, np.float32))
    F = gpu.csr_from_arrays(rows, rows, rp, ci, np.asarray(va, np.float32))
    assert gpu.csr_to_gpu(A) == 0 and gpu.csr_to_gpu(F) == 0
    d_b, d_x = gpu.CudaBuffer(4), gpu.CudaBuffer(4)
    d_b.copyFromHost(np.ones(4, np.float32), 4)
    x0 = np.array([7.0, -1.0, 2.5, 0.25], np.float32)
    d_x.copyFromHost(x0, 4)
    try:
        res = gpu.gmres_solve_lu(A, F, d_b, d_x, gpu.GMRESConfig(preconditioner=0))
        assert res.error_code == want, (case, res.error_code)
        assert np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
        # the same A with itself as the factor is fine (its diagonal is sound), and x moves
        res = gpu.gmres_solve_lu(A, A, d_b, d_x)
        assert res.error_code == 0 and res.converged == 1
        assert not np.array_equal(bits(d_x.copyToHost(4)), bits(x0))
    finally:
        gpu.csr_destroy(A)
        gpu.csr_destroy(F)
        d_b.release()
        d_x.release()


# ------------------------------------------------------------------------------------------ 9. engines, stop rules
def test_engines_agree(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)
    # ilu0_csr wants ascending columns: the factor comes with the convection-diffusion matrix only
    for matrix, kinds in ((nonsym.random_nonsym(3000, 7, seed=5, negative_rows=0.25), ("none", "jacobi")),
                          (nonsym.convdiff2d(64, 5.0), ("none", "jacobi", "lu"))):
        _engines_agree(gpu, matrix, kinds)


def _engines_agree(gpu, matrix, kinds):
    s = System(gpu, *matrix)
    try:
        F = s.factor() if "lu" in kinds else None
        for kind in kinds:
            cfg = dict(preconditioner=JACOBI if kind == "jacobi" else NONE, LU=F if kind == "lu" else None)
            for k in (3, 12):
                out = {}
                for engine in (0, 1, -1):               # 1 builds the plan, -1 then finds it cached
                    res, x = s.solve(tolerance=0.0, max_iterations=k, restart=8, engine=engine, **cfg)
                    assert (res.error_code, res.iterations, res.breakdown) == (0, k, 0), (kind, engine)
                    check_honest(s, res, x)
                    out[engine] = (float(res.relative_residual), s.bound(x))
                for engine in (1, -1):
                    assert abs(out[engine][0] - out[0][0]) <= SPREAD * out[0][0] + out[engine][1] + out[0][1], \
                        (kind, k, out)
            iters = [s.solve(tolerance=1e-5, restart=8, engine=engine, **cfg)[0].iterations for engine in (0, 1)]
            assert iters[0] == iters[1], (kind, iters)
        assert gpu.csr_has_tiled_plan(s.A)
    finally:
        s.close()


def test_max_iterations_zero_a_good_guess_and_a_zero_b(gpu, cd64):
    s = cd64
    x0 = np.full(s.n, 0.5, np.float32)
    res, x = s.solve(x0=x0, max_iterations=0)
    assert (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown) == (0, 0, 0, 0, 0)
    assert np.array_equal(bits(x), bits(x0))
    check_honest(s, res, x)
    res, x_solved = s.solve(tolerance=1e-5, engine=0)
    assert res.converged and res.iterations > 0
    check_honest(s, res, x_solved, 1e-5)
    res2, x2 = s.solve(x0=x_solved, tolerance=1e-3, engine=0)
    assert (res2.error_code, res2.converged, res2.iterations, res2.restarts, res2.breakdown) == (0, 1, 0, 0, 0)
    assert np.array_equal(bits(x2), bits(x_solved)) and res2.relative_residual <= 1e-3
    # the same solve capped at its own step count, and one past it: nothing enqueued after `done` moved x
    for extra in (0, 1):
        res_k, x_k = s.solve(tolerance=1e-5, engine=0, max_iterations=res.iterations + extra)
        assert res_k.iterations == res.iterations and res_k.converged and np.array_equal(bits(x_k), bits(x_solved))
    z = System(gpu, *nonsym.convdiff2d(16, 2.0), b=np.zeros(256, np.float32))
    try:
        res, x = z.solve(x0=np.full(z.n, 3.0, np.float32))
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0)
        assert np.array_equal(x, np.zeros(z.n, np.float32))
    finally:
        z.close()


# ------------------------------------------------------------------------------------------ 10. views
@pytest.mark.parametrize("m", [9, 17])
def test_b_and_x_as_views_into_larger_buffers(gpu, m):
    n, rp, ci, va = nonsym.convdiff2d(m, 3.0)               # 81 and 289 rows: no multiple of four
    s = System(gpu, n, rp, ci, va)
    try:
        F = s.factor()
        for kind in ("none", "jacobi", "lu"):
            cfg = gpu.GMRESConfig(tolerance=1e-6, restart=9, engine=0, preconditioner=JACOBI if kind == "jacobi" else 0)
            call = (lambda b, x: gpu.gmres_solve_lu(s.A, F, b, x, cfg)) if kind == "lu" else \
                (lambda b, x: gpu.gmres_solve(s.A, b, x, cfg))
            s.d_x.copyFromHost(np.zeros(n, np.float32), n)
            plain = call(s.d_b, s.d_x)
            x_plain = s.d_x.copyToHost(n)
            with av.Views(gpu) as views:
                v_b = views.x(s.b, 1)
                v_x = views.view(np.zeros(n, np.float32), 1, av.SENTINEL)
                res = call(v_b.ptr, v_x.ptr)
                assert (res.error_code, res.iterations, res.restarts, res.converged) == \
                    (0, plain.iterations, plain.restarts, 1), kind
                assert np.array_equal(bits(v_x.download()), bits(x_plain)), kind
                assert res.relative_residual == plain.relative_residual
                views.check_guards(kind)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ 11. C++ caller
def test_cpp_gmres_smoke(gpu, tmp_path):
    """tests/cpp/gmres_smoke.cpp through spmv/gmres.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "gmres_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "gmres_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
