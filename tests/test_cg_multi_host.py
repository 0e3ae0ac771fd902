"""cg_solve_multi (include/spmv/cg.h) on the host side (no GPU): the exported names and the argument checks that
come before any device work, in their documented order, through the C ABI and the Python wrapper.  Pairs of faults
show which check wins.  X and `results` are host memory standing in for device arrays, as in tests/test_cg_host.py:
a rejected call must leave X untouched and write nothing to `results` but error_code."""
import ctypes

import numpy as np

from test_cg_host import _device_header, _host_matrix

K_MAX = 32
POISON = np.float32(-7.25)


class Arrays:
    """Host stand-ins: B and X of `rows` x `ld` floats, far apart in one allocation, and `count` poisoned results."""

    def __init__(self, spmv, rows=8, ld=K_MAX + 1, count=K_MAX + 1):
        self.spmv = spmv
        self.store = np.full(4 * rows * ld, POISON, np.float32)
        self.B = self.store.ctypes.data
        self.X = self.B + 4 * 2 * rows * ld
        self.results = (spmv.CGResult * count)()
        for r in self.results:
            r.error_code, r.iterations, r.relative_residual = 12345, 77, 0.5
            r.converged, r.breakdown, r.elapsed_ms = 9, 9, 2.5

    def assert_untouched(self, written, code):
        assert np.all(self.store == POISON)
        for j, r in enumerate(self.results):
            assert r.error_code == (code if j < written else 12345), (j, r.error_code)
            assert (r.iterations, r.relative_residual, r.converged, r.breakdown, r.elapsed_ms) == (77, 0.5, 9, 9, 2.5)


def _c_call(spmv, A, B, ldb, X, ldx, k, cfg, results):
    return spmv.lib().spmv_c_cg_solve_multi(A, ctypes.c_void_p(B), ldb, ctypes.c_void_p(X), ldx, k,
                                            ctypes.byref(cfg) if cfg is not None else None, results)


def test_names_exist_in_the_c_abi_and_the_python_mirror(spmv):
    assert "spmv_c_cg_solve_multi" in spmv.EXPORTED_SYMBOLS
    assert hasattr(spmv.lib(), "spmv_c_cg_solve_multi")
    assert callable(spmv.cg_solve_multi)


def test_checks_in_the_stated_order_through_the_c_abi(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    A = _host_matrix(spmv)                        # square, host only: INVALID_FORMAT at check 6
    R = spmv.csr_create(5, 4, 0)                  # not square
    Z = spmv.csr_create(0, 0, 0)                  # empty
    D = _device_header(spmv)                      # passes 1..6
    try:
        def call(M, B, ldb, X, ldx, k, cfg, results, written):
            rc = _c_call(spmv, M, B, ldb, X, ldx, k, cfg, results)
            a.assert_untouched(written if results is not None else 0, rc)
            for r in a.results:
                r.error_code = 12345
            return rc

        # 1. nulls, before k (0 and 33 are bad), the leading dimensions, the shape, everything
        for k in (0, 4, K_MAX + 1):
            written = k if 1 <= k <= K_MAX else 0
            assert call(None, a.B, 1, a.X, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, None, 1, a.X, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, a.B, 1, None, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, a.B, 1, a.X, 1, k, bad_cfg, None, 0) == E.INVALID_ARGUMENT
        # 2. k, before the leading dimensions and the shape (INVALID_DIMENSION would win otherwise)
        for k in (0, -1, K_MAX + 1, 1 << 20):
            assert call(R, a.B, 40, a.X, 40, k, bad_cfg, a.results, 0) == E.INVALID_ARGUMENT
        # 3. leading dimensions, before the shape
        assert call(R, a.B, 3, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
        assert call(R, a.B, 4, a.X, 3, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
        assert call(Z, a.B, 0, a.X, 4, 1, bad_cfg, a.results, 1) == E.INVALID_ARGUMENT      # before the empty system
        # 4. not square, before the empty and format checks
        assert call(R, a.B, 4, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_DIMENSION
        R0 = spmv.csr_create(0, 3, 0)
        assert call(R0, a.B, 4, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_DIMENSION
        spmv.csr_destroy(R0)
        # 6. missing device arrays, before the config and the overlap
        assert call(A, a.B, 4, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_FORMAT
        assert call(A, a.B, 4, a.B, 4, 4, None, a.results, 4) == E.INVALID_FORMAT
        # 7. config values, before the overlap; engine 1 is rejected here, -1 and 0 are not
        for cfg in (spmv.CGConfig(tolerance=-1e-3), spmv.CGConfig(tolerance=float("nan")),
                    spmv.CGConfig(max_iterations=-1), spmv.CGConfig(preconditioner=2),
                    spmv.CGConfig(preconditioner=-1), spmv.CGConfig(engine=1), spmv.CGConfig(engine=2),
                    spmv.CGConfig(engine=-2)):
            assert call(D, a.B, 4, a.B, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
            assert call(D, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
        # 8. overlap of [B, B + (n - 1) ldb + k) and [X, X + (n - 1) ldx + k): n = 8, k = 3, ldb = 5 -> 38 floats of B,
        #    ldx = 4 -> 31 floats of X
        for cfg in (None, spmv.CGConfig(engine=0), spmv.CGConfig(engine=-1, preconditioner=0)):
            for x in (a.B, a.B + 4, a.B + 4 * 37, a.B - 4 * 30):
                assert call(D, a.B, 5, x, 4, 3, cfg, a.results, 3) == E.INVALID_ARGUMENT
    finally:
        for M in (A, R, Z, D):
            spmv.csr_destroy(M)


def test_the_same_order_through_python(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    A, R, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), _device_header(spmv)
    try:
        def codes(*args, **kw):
            out = spmv.cg_solve_multi(*args, **kw)
            assert np.all(a.store == POISON)
            assert isinstance(out, list) and len(out) >= 1
            assert len({r.error_code for r in out}) == 1
            assert all((r.iterations, r.converged, r.breakdown) == (0, 0, 0) for r in out)
            return out[0].error_code, len(out)

        assert codes(None, a.B, a.X, 0, config=bad_cfg) == (E.INVALID_ARGUMENT, 1)              # null before k
        assert codes(R, None, a.X, 4, ldb=1, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.B, None, 4, ldx=1, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.B, a.X, 0, config=bad_cfg) == (E.INVALID_ARGUMENT, 1)                 # k before the shape
        assert codes(R, a.B, a.X, K_MAX + 1, config=bad_cfg) == (E.INVALID_ARGUMENT, K_MAX + 1)
        assert codes(R, a.B, a.X, 4, ldb=3, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)          # ld before the shape
        assert codes(R, a.B, a.X, 4, ldx=3, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.B, a.X, 4, config=bad_cfg) == (E.INVALID_DIMENSION, 4)                # shape before format
        assert codes(A, a.B, a.B, 4, config=bad_cfg) == (E.INVALID_FORMAT, 4)                   # format before config
        assert codes(D, a.B, a.B, 4, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(D, a.B, a.X, 4, config=spmv.CGConfig(engine=1)) == (E.INVALID_ARGUMENT, 4)
        assert codes(D, a.B, a.B + 4 * 37, 3, ldb=5, ldx=4) == (E.INVALID_ARGUMENT, 3)          # overlap, good config
        assert codes(D, a.B, a.B - 4 * 30, 3, ldb=5, ldx=4, config=spmv.CGConfig(engine=0)) == (E.INVALID_ARGUMENT, 3)
    finally:
        for M in (A, R, D):
            spmv.csr_destroy(M)


def test_empty_system_gives_k_converged_results(spmv):
    """num_rows == 0 comes after the k / ld / shape checks and before the format, config and overlap checks."""
    E = spmv.SpMVError
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    Z = spmv.csr_create(0, 0, 0)
    try:
        for k in (1, 5, K_MAX):
            a = Arrays(spmv)
            assert _c_call(spmv, Z, a.B, k, a.B, k, k, bad_cfg, a.results) == E.SUCCESS
            assert np.all(a.store == POISON)
            for j, r in enumerate(a.results):
                if j < k:
                    assert (r.error_code, r.iterations, r.converged, r.breakdown) == (E.SUCCESS, 0, 1, 0)
                    assert r.relative_residual == 0.0 and r.elapsed_ms == 0.0
                else:
                    assert (r.error_code, r.iterations, r.converged) == (12345, 77, 9)
            out = spmv.cg_solve_multi(Z, a.B, a.B, k, config=bad_cfg)
            assert len(out) == k
            assert all((r.error_code, r.iterations, r.converged, r.breakdown) == (E.SUCCESS, 0, 1, 0) for r in out)
    finally:
        spmv.csr_destroy(Z)
