"""gmres_solve / gmres_solve_lu (csrc/gmres.hip) held to the bit on exact data.

tests/test_gpu_gmres.py compares the solver with the numpy restatement by measured bounds, which fits random data
and cannot see one wrong bit.  Here the data are built so that the restatement's bits ARE the device's:

* the one-hot Krylov systems of exact_data.ONEHOT_CASES walk the whole basis (every group-of-eight boundary of the
  restart, the masked tails of the 16-byte loads, the second trip of fold_columns' lane loop, of the basis kernels'
  grid stride, of the element-wise kernels and of the row loops of gmres_spmv<1> / gmres_residual<1>, and a cycle that
  closes before the host expects it);
* the first step of every lane count's integer system under a +-1 / 0 right-hand side is predictable from integer
  arithmetic (exact_data.gmres_first_step).

tests/test_exact_data.py proves every claim about the data without a GPU.

Tolerances.  x: none (0 ulp) everywhere.  iterations, restarts, converged, breakdown: equal.  relative_residual of the
one-hot runs: 1 fp32 ulp of the restatement's, because r.r at a close sums up to iterations + 1 fp64 terms of mixed
exponent whose last fp64 bit depends on the order of the sum, and the square root, the division by ||b|| = 4 (exact)
and the rounding to fp32 can carry that bit into the last fp32 bit and no further.  relative_residual of the first
step: test_gpu_gmres.check_honest (its SpMV A x1 is not exact)."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import gmres_cases as gc

pytestmark = pytest.mark.gpu

gmres_tests = importlib.import_module("test_gpu_gmres")
sweep = importlib.import_module("test_gpu_lane_sweep")
System, check_honest, bits = gmres_tests.System, gmres_tests.check_honest, gmres_tests.bits
assert_bits = sweep.assert_bits
NONE, JACOBI = gc.NONE, gc.JACOBI


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def assert_onehot(s, system, case, res, x, want, what):
    x_ref, it, restarts, conv, brk, rel = want
    print(what, "iterations", res.iterations, it, "residual", res.relative_residual, rel)
    assert res.error_code == 0, what
    assert (res.iterations, res.restarts, res.converged, res.breakdown) == (it, restarts, int(conv), brk), what
    bad = np.flatnonzero(bits(x) != bits(x_ref))
    walk = system["walk"].tolist()
    assert bad.size == 0, (what, [(int(i), walk.index(int(i)) if int(i) in walk else None, float(x[i]),
                                   float(x_ref[i])) for i in bad[:8]])
    assert ulps(res.relative_residual, rel) <= 1, (what, res.relative_residual, rel)


@pytest.mark.parametrize("name", ed.ONEHOT_NAMES)
def test_onehot_system_walks_the_basis_bit_for_bit(gpu, name):
    """tolerance 0 and a fixed step count, NONE and JACOBI, against the restatement on the walk positions
    (exact_data.gmres_onehot_reference); then gmres_solve_lu with the factor D = diag(A), whose two triangular solves
    divide by powers of two: JACOBI's bits through gmres_add and the stored u."""
    case, system = ed.onehot_case(name)
    n = system["n"]
    s = System(gpu, n, system["rp"], system["ci"], system["va"], b=system["b"])
    idx = np.arange(n, dtype=np.int32)
    D = gpu.csr_from_arrays(n, n, np.arange(n + 1, dtype=np.int32), idx, system["d"])
    assert gpu.csr_to_gpu(D) == 0
    try:
        cfg = dict(tolerance=0.0, max_iterations=case["max_iterations"], restart=case["restart"], engine=0)
        for precond in (NONE, JACOBI):
            want = ed.gmres_onehot_reference(system, case["restart"], case["max_iterations"], precond)
            res, x = s.solve(preconditioner=precond, **cfg)
            assert_onehot(s, system, case, res, x, want, (name, precond))
        res, x = s.solve(LU=D, **cfg)
        assert_onehot(s, system, case, res, x, want, (name, "lu = diag(A)"))
        assert not gpu.csr_has_tiled_plan(s.A)
    finally:
        gpu.csr_destroy(D)
        s.close()


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_gmres_first_step_is_predictable_to_the_bit(gpu, name):
    """gmres_spmv<L> and the three basis kernels on the integer non-symmetric system of each L with b = +-1 on 1024
    rows: x1 == fp32(y_0) b / 32 with y_0 from int64 / float64 arithmetic (exact_data.gmres_first_step, which asserts
    every step of the derivation).  One wrong entry of A b moves b.A b or w.w by an integer, far more than fp32(y_0)
    resolves.  The equality assumes correctly rounded fp64 sqrt and division on the device."""
    L, n, rp, ci, va, b = ed.gmres_step_system(name)
    want, y0 = ed.gmres_first_step(rp, ci, va, b, ed.GMRES_STEP_K)
    s = System(gpu, n, rp, ci, va, b=b)
    try:
        res, x = s.solve(tolerance=0.0, max_iterations=1, preconditioner=NONE, engine=0)
        what = (name, L, float(y0), res.iterations)
        assert (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown) == (0, 1, 0, 0, 0), what
        assert_bits(rp, x, want, what)
        check_honest(s, res, x)
    finally:
        s.close()
