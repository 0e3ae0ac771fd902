"""gmres_solve / gmres_solve_lu (include/spmv/gmres.h) on the host side (no GPU): the exported names, the struct
layouts and defaults, the argument checks that come before any device work, in their documented order, through the C
ABI and the Python wrapper, and the numpy restatement of the header's rules (tests/gmres_cases.py) against fp64."""
import ctypes

import numpy as np
import pytest

import gmres_cases as gc


def _host_matrix(spmv, rows=8, cols=8):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, i % cols] = -4.0
        dense[i, (i + 1) % cols] = 1.0
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


# fake, never-dereferenced device addresses: every call below must return before it touches them
B, X = 0x100000, 0x200000
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def _device_header(spmv, n=8, nnz=16):
    return spmv.csr_wrap_device(n, n, nnz, FAKE_RP, FAKE_CI, FAKE_VA)


def test_names_exist_in_the_c_abi_the_library_and_python(spmv):
    for name in ("spmv_c_gmres_solve", "spmv_c_gmres_solve_lu"):
        assert name in spmv.EXPORTED_SYMBOLS
        assert hasattr(spmv.lib(), name)
    assert callable(spmv.gmres_solve) and callable(spmv.gmres_solve_lu)
    assert (spmv.GMRES_NO_BREAKDOWN, spmv.GMRES_SINGULAR, spmv.GMRES_NOT_FINITE) == (0, 1, 2)
    R = spmv.GMRESResult
    assert (R.NONE, R.SINGULAR, R.NOT_FINITE) == (0, 1, 2)
    assert (spmv.GMRESConfig.NONE, spmv.GMRESConfig.JACOBI) == (spmv.CGConfig.NONE, spmv.CGConfig.JACOBI)
    assert (gc.NO_BREAKDOWN, gc.SINGULAR, gc.NOT_FINITE) == (R.NONE, R.SINGULAR, R.NOT_FINITE)


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R = spmv.GMRESConfig, spmv.GMRESResult
    assert ctypes.sizeof(C) == 20 and ctypes.sizeof(R) == 28
    assert [f for f, _ in C._fields_] == ["tolerance", "max_iterations", "restart", "preconditioner", "engine"]
    assert [f for f, _ in R._fields_] == ["error_code", "iterations", "restarts", "relative_residual", "converged",
                                          "breakdown", "elapsed_ms"]
    assert (C.tolerance.offset, C.max_iterations.offset, C.restart.offset, C.preconditioner.offset,
            C.engine.offset) == (0, 4, 8, 12, 16)
    assert (R.error_code.offset, R.iterations.offset, R.restarts.offset, R.relative_residual.offset,
            R.converged.offset, R.breakdown.offset, R.elapsed_ms.offset) == (0, 4, 8, 12, 16, 20, 24)
    c = C()
    assert (np.float32(c.tolerance), c.max_iterations, c.restart, c.preconditioner, c.engine) == \
        (np.float32(1e-6), 1000, 30, 1, -1)
    r = R()
    assert (r.error_code, r.iterations, r.restarts, r.converged, r.breakdown) == (0, 0, 0, 0, 0)


def _c_call(spmv, A, b, x, cfg):
    out = spmv.GMRESResult(error_code=12345)
    rc = spmv.lib().spmv_c_gmres_solve(A, ctypes.c_void_p(b), ctypes.c_void_p(x),
                                       ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def _c_call_lu(spmv, A, LU, b, x, cfg):
    out = spmv.GMRESResult(error_code=12345)
    rc = spmv.lib().spmv_c_gmres_solve_lu(A, LU, ctypes.c_void_p(b), ctypes.c_void_p(x),
                                          ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_checks_in_the_stated_order_through_the_c_abi_and_python(spmv):
    E = spmv.SpMVError
    Cfg = spmv.GMRESConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, b, x, cfg=None: _c_call(spmv, A, b, x, cfg),
                 lambda A, b, x, cfg=None: spmv.gmres_solve(A, b, x, cfg)):
        A = _host_matrix(spmv)
        # 1. nulls, before everything else
        assert call(None, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, None, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, B, None, bad_cfg).error_code == E.INVALID_ARGUMENT
        # 2. not square, before the empty and format checks
        for rows, cols in ((0, 3), (5, 4)):
            R = spmv.csr_create(rows, cols, 0)
            assert call(R, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
            spmv.csr_destroy(R)
        # 3. empty system: converged after 0 iterations, whatever the config and even with b and x the same
        Z = spmv.csr_create(0, 0, 0)
        res = call(Z, B, B, bad_cfg)
        assert (res.error_code, res.converged, res.iterations, res.restarts, res.breakdown) == (E.SUCCESS, 1, 0, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (host-only matrix), before the config and the overlap check
        assert call(A, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        assert call(A, B, B).error_code == E.INVALID_FORMAT
        for rp, ci, va in ((FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
            D = spmv.csr_wrap_device(8, 8, 16, rp, ci, va)
            assert call(D, B, X).error_code == E.INVALID_FORMAT
            spmv.csr_destroy(D)
        # 5. config values, restart among them, before the overlap check
        D = _device_header(spmv)
        for cfg in (Cfg(tolerance=-1e-3), Cfg(tolerance=float("nan")), Cfg(max_iterations=-1), Cfg(restart=0),
                    Cfg(restart=-3), Cfg(restart=65), Cfg(preconditioner=2), Cfg(preconditioner=-1), Cfg(engine=2),
                    Cfg(engine=-2)):
            assert call(D, B, B, cfg).error_code == E.INVALID_ARGUMENT
            assert call(D, B, X, cfg).error_code == E.INVALID_ARGUMENT
        # 6. overlapping b and x ranges (8 floats = 32 bytes each); restart 1 and 64 are accepted values
        for x in (B, B + 4, B + 28, B - 28):
            assert call(D, B, x).error_code == E.INVALID_ARGUMENT
            assert call(D, B, x, Cfg(preconditioner=0, engine=0, restart=1)).error_code == E.INVALID_ARGUMENT
            assert call(D, B, x, Cfg(restart=64)).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_lu_checks_in_the_stated_order(spmv):
    E = spmv.SpMVError
    Cfg = spmv.GMRESConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, LU, b, x, cfg=None: _c_call_lu(spmv, A, LU, b, x, cfg),
                 lambda A, LU, b, x, cfg=None: spmv.gmres_solve_lu(A, LU, b, x, cfg)):
        A = _host_matrix(spmv)
        D = _device_header(spmv)
        # null LU with the other nulls
        assert call(D, None, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(None, D, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        # A's own dimension check first, then LU's: not square, or another size
        R = spmv.csr_create(5, 4, 0)
        assert call(R, D, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
        assert call(D, R, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
        spmv.csr_destroy(R)
        D9 = _device_header(spmv, n=9)
        assert call(D, D9, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
        spmv.csr_destroy(D9)
        # LU without device arrays, with A's format check and before the config
        assert call(D, A, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        assert call(A, D, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        # config: the preconditioner field is not read, restart is
        assert call(D, D, B, B, Cfg(restart=65)).error_code == E.INVALID_ARGUMENT
        assert call(D, D, B, X, Cfg(restart=0, preconditioner=7)).error_code == E.INVALID_ARGUMENT
        # overlap (an unknown preconditioner value does not matter here)
        assert call(D, D, B, B + 4, Cfg(preconditioner=7)).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_error_code_is_written_through_out_and_out_may_be_null(spmv):
    A = _host_matrix(spmv)
    out = spmv.GMRESResult(error_code=7, iterations=9, restarts=3, breakdown=2)
    assert spmv.lib().spmv_c_gmres_solve(A, ctypes.c_void_p(B), None, None, ctypes.byref(out)) == \
        spmv.SpMVError.INVALID_ARGUMENT
    assert (out.error_code, out.iterations, out.restarts, out.breakdown) == (spmv.SpMVError.INVALID_ARGUMENT, 0, 0, 0)
    assert spmv.lib().spmv_c_gmres_solve(A, ctypes.c_void_p(B), ctypes.c_void_p(X), None, None) == \
        spmv.SpMVError.INVALID_FORMAT
    spmv.csr_destroy(A)


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(gc.SYSTEMS))
def test_restatement_reports_its_recomputed_residual_and_is_near_the_fp64_optimum(name):
    """After k <= restart steps from x0 = 0 the restatement's true residual (fp64, from its fp32 x) may exceed the
    fp64 least-squares optimum over the same Krylov space only by rounding.  Measured over these systems, NONE and
    JACOBI, (restart, k) in (8, 1), (8, 3), (8, 8), (30, 1), (30, 3), (30, 8), (30, 20): the worst relative excess is
    9.9e-5 (random_64, JACOBI, k = 8, residual 1.3e-4) and the worst absolute one 1.5e-7.  The assertion allows twice
    both."""
    n, rp, ci, va = gc.SYSTEMS[name]()
    b = gc.rhs(n)
    for precond in (gc.NONE, gc.JACOBI):
        for restart, k in ((8, 1), (8, 8), (30, 20)):
            x, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, k, restart, precond)
            assert it <= k and brk == gc.NO_BREAKDOWN      # n < k: lucky breakdowns, then cycles of their own
            assert restarts == 0 or n < k
            true = gc.true_residual(rp, ci, va, b, x)
            # reported == recomputed by construction: the fp32 route against fp64, to one SpMV's rounding
            assert abs(rel - true) <= gc.residual_rounding_bound(rp, ci, va, b, x), (name, precond, k, rel, true)
            opt = gc.krylov_optimum(n, rp, ci, va, b, it, precond)
            print(name, precond, restart, k, "true", true, "optimum", opt)
            assert true <= opt * (1 + 2e-4) + 3e-7, (name, precond, restart, k, true, opt)


def test_restatement_restart_is_a_new_solve_and_the_residual_never_grows():
    n, rp, ci, va = gc.SYSTEMS["convdiff2d_16"]()
    b = gc.rhs(n)
    m = 7
    one = gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, 2 * m, m, gc.JACOBI)
    first = gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, m, m, gc.JACOBI)
    second = gc.restate(n, rp, ci, va, b, first[0], 0.0, m, m, gc.JACOBI)
    assert np.array_equal(one[0].view(np.uint32), second[0].view(np.uint32)) and one[5] == second[5]
    assert (one[1], one[2], first[1], second[1]) == (2 * m, 1, m, m)
    rels = [gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, k, m, gc.JACOBI)[5] for k in range(0, 2 * m + 1)]
    bound = gc.residual_rounding_bound(rp, ci, va, b, one[0])
    assert all(later <= earlier + 2 * bound for earlier, later in zip(rels, rels[1:])), rels


def test_restatement_edge_cases():
    # lucky breakdown: diagonal powers of two, b = 2^k e_1
    n = 6
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    va = np.array([4, -2, 0.5, 8, 1, -16], np.float32)
    b = np.zeros(n, np.float32)
    b[0] = 32.0
    for precond in (gc.NONE, gc.JACOBI):
        x, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, b, np.zeros(n), 1e-6, 100, 30, precond)
        assert (it, restarts, conv, brk, rel) == (1, 0, True, gc.NO_BREAKDOWN, 0.0)
        assert np.array_equal(x, np.array([8, 0, 0, 0, 0, 0], np.float32))
    # SINGULAR: a zero row and column that b reaches
    rp, ci, va = np.array([0, 1, 1], np.int32), np.array([0], np.int32), np.array([2.0], np.float32)
    x, it, restarts, conv, brk, rel = gc.restate(2, rp, ci, va, np.array([0, 1], np.float32),
                                                 np.array([0, 5], np.float32), 1e-6, 100, 30, gc.NONE)
    assert (it, conv, brk) == (0, False, gc.SINGULAR) and np.array_equal(x, np.array([0, 5], np.float32))
    # NOT_FINITE: an inf in b, x left at the guess
    n, rp, ci, va = gc.SYSTEMS["random_63"]()
    b = gc.rhs(n)
    b[5] = np.inf
    x0 = np.full(n, 0.25, np.float32)
    x, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, b, x0, 1e-6, 100, 30, gc.JACOBI)
    assert (it, conv, brk) == (0, False, gc.NOT_FINITE) and np.array_equal(x, x0)
    # max_iterations = 0: the guess with its residual
    b = gc.rhs(n)
    x, it, restarts, conv, brk, rel = gc.restate(n, rp, ci, va, b, x0, 1e-6, 0, 30, gc.JACOBI)
    assert (it, conv, brk) == (0, False, 0) and np.array_equal(x, x0)
    assert abs(rel - gc.true_residual(rp, ci, va, b, x0)) <= gc.residual_rounding_bound(rp, ci, va, b, x0)
