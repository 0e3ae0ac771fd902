"""bicgstab_solve (include/spmv/bicgstab.h) on the host side (no GPU): the exported names, the struct layouts and
defaults, and the argument checks that come before any device work, in their documented order, through the C ABI
and the Python wrapper."""
import ctypes

import numpy as np


def _host_matrix(spmv, rows=8, cols=8):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, i % cols] = -4.0                   # negative diagonal: fine for BiCGSTAB
        dense[i, (i + 1) % cols] = 1.0
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


# fake, never-dereferenced device addresses: every call below must return before it touches them
B, X = 0x100000, 0x200000
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def _device_header(spmv, n=8, nnz=16):
    return spmv.csr_wrap_device(n, n, nnz, FAKE_RP, FAKE_CI, FAKE_VA)


def test_names_exist_in_the_c_abi_the_library_and_python(spmv):
    assert "spmv_c_bicgstab_solve" in spmv.EXPORTED_SYMBOLS
    assert hasattr(spmv.lib(), "spmv_c_bicgstab_solve")
    assert callable(spmv.bicgstab_solve)
    assert (spmv.BICGSTAB_NO_BREAKDOWN, spmv.BICGSTAB_RHO, spmv.BICGSTAB_ALPHA, spmv.BICGSTAB_OMEGA) == (0, 1, 2, 3)
    R = spmv.BiCGStabResult
    assert (R.NONE, R.RHO, R.ALPHA, R.OMEGA) == (0, 1, 2, 3)
    assert (spmv.BiCGStabConfig.NONE, spmv.BiCGStabConfig.JACOBI) == (spmv.CGConfig.NONE, spmv.CGConfig.JACOBI)


def test_struct_sizes_offsets_and_defaults(spmv):
    assert ctypes.sizeof(spmv.BiCGStabConfig) == 16
    assert ctypes.sizeof(spmv.BiCGStabResult) == 24
    assert [f for f, _ in spmv.BiCGStabConfig._fields_] == ["tolerance", "max_iterations", "preconditioner",
                                                            "engine"]
    assert [f for f, _ in spmv.BiCGStabResult._fields_] == ["error_code", "iterations", "relative_residual",
                                                            "converged", "breakdown", "elapsed_ms"]
    C, R = spmv.BiCGStabConfig, spmv.BiCGStabResult
    assert (C.tolerance.offset, C.max_iterations.offset, C.preconditioner.offset, C.engine.offset) == (0, 4, 8, 12)
    assert (R.error_code.offset, R.iterations.offset, R.relative_residual.offset, R.converged.offset,
            R.breakdown.offset, R.elapsed_ms.offset) == (0, 4, 8, 12, 16, 20)
    c = spmv.BiCGStabConfig()
    assert (np.float32(c.tolerance), c.max_iterations, c.preconditioner, c.engine) == (np.float32(1e-6), 1000, 1, -1)
    r = spmv.BiCGStabResult()
    assert (r.error_code, r.iterations, r.converged, r.breakdown) == (0, 0, 0, 0)


def _c_call(spmv, A, b, x, cfg):
    out = spmv.BiCGStabResult(error_code=12345)
    rc = spmv.lib().spmv_c_bicgstab_solve(A, ctypes.c_void_p(b), ctypes.c_void_p(x),
                                          ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_checks_in_the_stated_order_through_the_c_abi_and_python(spmv):
    E = spmv.SpMVError
    Cfg = spmv.BiCGStabConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, b, x, cfg=None: _c_call(spmv, A, b, x, cfg),
                 lambda A, b, x, cfg=None: spmv.bicgstab_solve(A, b, x, cfg)):
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
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (E.SUCCESS, 1, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (host-only matrix), before the config and the overlap check
        assert call(A, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        assert call(A, B, B).error_code == E.INVALID_FORMAT
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
        assert call(D, B, X).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(D)
        D = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, None)
        assert call(D, B, X).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(D)
        # 5. config values, before the overlap check
        D = _device_header(spmv)
        for cfg in (Cfg(tolerance=-1e-3), Cfg(tolerance=float("nan")), Cfg(max_iterations=-1),
                    Cfg(preconditioner=2), Cfg(preconditioner=-1), Cfg(engine=2), Cfg(engine=-2)):
            assert call(D, B, B, cfg).error_code == E.INVALID_ARGUMENT
            assert call(D, B, X, cfg).error_code == E.INVALID_ARGUMENT
        # 6. overlapping b and x ranges (8 floats = 32 bytes each)
        for x in (B, B + 4, B + 28, B - 28):
            assert call(D, B, x).error_code == E.INVALID_ARGUMENT
            assert call(D, B, x, Cfg(preconditioner=0, engine=0)).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_error_code_is_written_through_out_and_out_may_be_null(spmv):
    A = _host_matrix(spmv)
    out = spmv.BiCGStabResult(error_code=7, iterations=9, breakdown=2)
    assert spmv.lib().spmv_c_bicgstab_solve(A, ctypes.c_void_p(B), None, None, ctypes.byref(out)) == \
        spmv.SpMVError.INVALID_ARGUMENT
    assert out.error_code == spmv.SpMVError.INVALID_ARGUMENT and out.iterations == 0 and out.breakdown == 0
    assert spmv.lib().spmv_c_bicgstab_solve(A, ctypes.c_void_p(B), ctypes.c_void_p(X), None, None) == \
        spmv.SpMVError.INVALID_FORMAT
    spmv.csr_destroy(A)
