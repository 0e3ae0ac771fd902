"""sptrsv_csr_multi / sptrsv_cpu_csr_multi / cg_solve_multi_ic (include/spmv/sptrsv.h, include/spmv/cg.h) on the host
side (no GPU): the exported names; sptrsv_cpu_csr_multi column by column against sptrsv_cpu_csr, bit for bit, with
leading dimensions, poisoned padding, in place and a zero diagonal; the argument checks of all four entry points that
come before any device work, in their documented order, through the C ABI and Python, with nothing written on
rejection; and the sanitized caller of the host code."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_cg_host import _device_header, _host_matrix
from test_cg_multi_host import Arrays, K_MAX, POISON

NAMES = ("sptrsv_csr_multi", "sptrsv_csr_multi_async", "sptrsv_cpu_csr_multi")
ALL_K = (1, 3, 4, 5, 8, 9, 32)

# fake, never-dereferenced device addresses of a factor matrix
FAKE_RP, FAKE_CI, FAKE_L = 0x300000, 0x400000, 0x900000


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


@pytest.fixture(scope="module")
def nonsym():
    return importlib.import_module("gpu-spmv_amd.nonsym")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _assert_same_bits(got, want, tag):
    """bit for bit; a NaN must meet a NaN, whose sign and payload IEEE 754 leaves open"""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(tag))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(_bits(got)[keep], _bits(want)[keep], err_msg=str(tag))


# ---- names ---------------------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)                     # what test_host_library.py checks
    cxx = open(os.path.join(ROOT, "include", "spmv", "sptrsv.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in declared and "spmv_c_" + name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), "spmv_c_" + name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name
    assert "spmv_c_cg_solve_multi_ic" in declared and hasattr(spmv.lib(), "spmv_c_cg_solve_multi_ic")
    assert callable(spmv.cg_solve_multi_ic)
    assert re.search(r"\bcg_solve_multi_ic\s*\(", open(os.path.join(ROOT, "include", "spmv", "cg.h")).read())


# ---- the host substitution -----------------------------------------------------------------------------------
def _cpu_multi(spmv, A, B, ldb, ldx, cfg, in_place=False):
    """X (n x k) of sptrsv_cpu_csr_multi through the C ABI on arrays with leading dimensions and poisoned padding that
    end at the last row's column k; asserts that the padding and B come back bit for bit."""
    n, k = B.shape
    hb = np.full((n - 1) * ldb + k, POISON, np.float32)
    for j in range(k):
        hb[j::ldb][:n] = B[:, j]
    if in_place:
        assert ldb == ldx
        hx = hb
    else:
        hx = np.full((n - 1) * ldx + k, POISON, np.float32)
    before = hb.copy()
    assert spmv.lib().spmv_c_sptrsv_cpu_csr_multi(A, _ptr(hb), ldb, _ptr(hx), ldx, k, ctypes.byref(cfg)) == 0
    X = np.stack([hx[j::ldx][:n] for j in range(k)], axis=1)
    pad = np.ones(hx.size, bool)
    for j in range(k):
        pad[j::ldx] = False
    assert np.array_equal(_bits(hx[pad]), _bits(np.full(int(pad.sum()), POISON, np.float32))), "padding written"
    if not in_place:
        assert np.array_equal(_bits(hb), _bits(before)), "B written"
    return X


def test_cpu_multi_equals_the_single_solve_column_by_column(spmv, spd, nonsym):
    rng = np.random.default_rng(17)
    nz, rpz, ciz, vaz = spd.poisson2d(12)
    vaz = vaz.copy()
    rz = np.repeat(np.arange(nz), np.diff(rpz))
    vaz[(ciz == rz) & (rz == 40)] = 0.0                               # a stored zero diagonal
    cases = {"poisson2d(14)": spd.poisson2d(14), "random_spd": spd.random_spd(300, 9, 4),
             "random_nonsym": nonsym.random_nonsym(350, 7, 2), "zero_diagonal": (nz, rpz, ciz, vaz)}
    for name, (n, rp, ci, va) in cases.items():
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        for k in ALL_K:
            B = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
            if name == "zero_diagonal":
                B[:, 0] = 0.0                                         # column 0 meets 0 / 0, the others x / 0
            for uplo in (0, 1):
                for unit in (0, 1):
                    cfg = spmv.SpTRSVConfig(uplo=uplo, diag=unit)
                    with np.errstate(all="ignore"):
                        want = np.stack([spmv.sptrsv_cpu_csr(A, B[:, j].copy(), cfg) for j in range(k)], axis=1)
                    tag = (name, k, uplo, unit)
                    for ldb, ldx, in_place in ((k, k, False), (k + 3, k + 1, False), (k + 2, k + 2, True),
                                               (k, k, True)):
                        got = _cpu_multi(spmv, A, B, ldb, ldx, cfg, in_place)
                        _assert_same_bits(got, want, tag + (ldb, ldx, in_place))
                    np.testing.assert_array_equal(_bits(spmv.sptrsv_cpu_csr_multi(A, B, cfg))[~np.isnan(want)],
                                                  _bits(want)[~np.isnan(want)], err_msg=str(tag))
                    if name == "zero_diagonal" and uplo == 0 and unit == 0:
                        assert np.isnan(want[40, 0]) and (k == 1 or np.isinf(want[40, 1:]).all()), tag
                        assert np.isfinite(want[:40]).all(), tag
        spmv.csr_destroy(A)


def test_an_inf_or_nan_stays_in_its_column(spmv, spd):
    n, rp, ci, va = spd.poisson2d(10)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    B = np.random.default_rng(2).uniform(0.5, 1.0, (n, 5)).astype(np.float32)
    clean = spmv.sptrsv_cpu_csr_multi(A, B)
    B2 = B.copy()
    B2[:, 1] = np.nan
    B2[3, 3] = np.inf
    with np.errstate(all="ignore"):
        got = spmv.sptrsv_cpu_csr_multi(A, B2)
    assert np.isnan(got[:, 1]).all() and not np.isfinite(got[3:, 3]).all()
    for j in (0, 2, 4):
        np.testing.assert_array_equal(_bits(got[:, j]), _bits(clean[:, j]))
    spmv.csr_destroy(A)


def test_cpu_multi_rejections_leave_x_untouched(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    A = _host_matrix(spmv)                                            # 8 x 8, every diagonal stored
    R = spmv.csr_create(5, 4, 0)
    store = np.full(4 * 8 * (K_MAX + 1), POISON, np.float32)
    Bp, Xp = store.ctypes.data, store.ctypes.data + 4 * 2 * 8 * (K_MAX + 1)
    bad_cfg = spmv.SpTRSVConfig(uplo=5)

    def call(M, b, ldb, x, ldx, k, cfg=None):
        rc = lib.spmv_c_sptrsv_cpu_csr_multi(M, ctypes.c_void_p(b), ldb, ctypes.c_void_p(x), ldx, k,
                                             ctypes.byref(cfg) if cfg is not None else None)
        assert np.all(store == POISON)
        return rc

    assert call(None, Bp, 1, Xp, 1, 0, bad_cfg) == E.INVALID_ARGUMENT
    assert call(R, None, 1, Xp, 1, 0, bad_cfg) == E.INVALID_ARGUMENT
    assert call(R, Bp, 1, None, 1, 0, bad_cfg) == E.INVALID_ARGUMENT
    for k in (0, -1, K_MAX + 1):
        assert call(R, Bp, 40, Xp, 40, k, bad_cfg) == E.INVALID_ARGUMENT          # k before the shape
    assert call(R, Bp, 3, Xp, 4, 4, bad_cfg) == E.INVALID_ARGUMENT                # ld before the shape
    assert call(R, Bp, 4, Xp, 3, 4, bad_cfg) == E.INVALID_ARGUMENT
    assert call(R, Bp, 4, Xp, 4, 4, bad_cfg) == E.INVALID_DIMENSION
    assert call(A, Bp, 4, Xp, 4, 4, bad_cfg) == E.INVALID_ARGUMENT                # the config
    for x in (Bp + 4, Bp + 4 * 37, Bp - 4 * 30):                                  # n = 8, k = 3: 38 and 31 floats
        assert call(A, Bp, 5, x, 4, 3) == E.INVALID_ARGUMENT
    assert call(A, Bp, 5, Bp, 4, 3) == E.INVALID_ARGUMENT                         # the same array, another ld
    with pytest.raises(ValueError):
        spmv.sptrsv_cpu_csr_multi(R, np.ones((5, 2), np.float32))
    for M in (A, R):
        spmv.csr_destroy(M)


# ---- the device entry points: checks before any device work --------------------------------------------------
def _c_multi(spmv, A, b, ldb, x, ldx, k, cfg):
    out = spmv.SpTRSVResult(error_code=12345)
    rc = spmv.lib().spmv_c_sptrsv_csr_multi(A, ctypes.c_void_p(b), ldb, ctypes.c_void_p(x), ldx, k,
                                            ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def _c_multi_async(spmv, A, b, ldb, x, ldx, k, cfg):
    rc = spmv.lib().spmv_c_sptrsv_csr_multi_async(A, ctypes.c_void_p(b), ldb, ctypes.c_void_p(x), ldx, k,
                                                  ctypes.byref(cfg) if cfg is not None else None, None)
    return spmv.SpTRSVResult(error_code=rc)


def test_sptrsv_multi_checks_in_the_stated_order(spmv):
    """B and X are host memory standing in for device arrays, as in tests/test_cg_multi_host.py: every call returns
    before it touches them, and they come back untouched."""
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.SpTRSVConfig(uplo=7)
    calls = (lambda M, b, ldb, x, ldx, k, cfg=None: _c_multi(spmv, M, b, ldb, x, ldx, k, cfg),
             lambda M, b, ldb, x, ldx, k, cfg=None: spmv.sptrsv_csr_multi(M, b, x, k, ldb, ldx, cfg),
             lambda M, b, ldb, x, ldx, k, cfg=None: _c_multi_async(spmv, M, b, ldb, x, ldx, k, cfg),
             lambda M, b, ldb, x, ldx, k, cfg=None: spmv.SpTRSVResult(
                 error_code=spmv.sptrsv_csr_multi_async(M, b, x, k, ldb, ldx, cfg)))
    A, R, Z, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), spmv.csr_create(0, 0, 0), _device_header(spmv)
    try:
        for raw in calls:
            def call(*args, **kw):
                res = raw(*args, **kw)
                assert np.all(a.store == POISON)
                return res.error_code
            # 1. nulls, before k, the leading dimensions and the shape
            for k in (0, 4, K_MAX + 1):
                assert call(None, a.B, 1, a.X, 1, k, bad_cfg) == E.INVALID_ARGUMENT
                assert call(R, None, 1, a.X, 1, k, bad_cfg) == E.INVALID_ARGUMENT
                assert call(R, a.B, 1, None, 1, k, bad_cfg) == E.INVALID_ARGUMENT
            # 2. k, before the leading dimensions and the shape (INVALID_DIMENSION would win otherwise)
            for k in (0, -1, K_MAX + 1, 1 << 20):
                assert call(R, a.B, 40, a.X, 40, k, bad_cfg) == E.INVALID_ARGUMENT
            # 3. leading dimensions, before the shape and the empty system
            assert call(R, a.B, 3, a.X, 4, 4, bad_cfg) == E.INVALID_ARGUMENT
            assert call(R, a.B, 4, a.X, 3, 4, bad_cfg) == E.INVALID_ARGUMENT
            assert call(Z, a.B, 0, a.X, 4, 1, bad_cfg) == E.INVALID_ARGUMENT
            # 4. sptrsv_csr's: not square; the empty system (SUCCESS whatever the config and the overlap)
            assert call(R, a.B, 4, a.X, 4, 4, bad_cfg) == E.INVALID_DIMENSION
            assert call(Z, a.B, 4, a.B + 4, 4, 4, bad_cfg) == E.SUCCESS
            # missing device arrays, before the config and the overlap
            assert call(A, a.B, 4, a.X, 4, 4, bad_cfg) == E.INVALID_FORMAT
            assert call(A, a.B, 4, a.B + 4, 4, 4) == E.INVALID_FORMAT
            # config ranges, before the overlap
            for cfg in (spmv.SpTRSVConfig(uplo=2), spmv.SpTRSVConfig(uplo=-1), spmv.SpTRSVConfig(diag=2),
                        spmv.SpTRSVConfig(ordered=2), spmv.SpTRSVConfig(ordered=-1)):
                assert call(D, a.B, 4, a.B + 4, 4, 4, cfg) == E.INVALID_ARGUMENT
                assert call(D, a.B, 4, a.X, 4, 4, cfg) == E.INVALID_ARGUMENT
            # overlap of [B, B + (n - 1) ldb + k) and [X, X + (n - 1) ldx + k): n = 8, k = 3, ldb = 5 -> 38 floats of
            # B, ldx = 4 -> 31 floats of X; the same array with two leading dimensions is one of them
            for cfg in (None, spmv.SpTRSVConfig(uplo=1, diag=1, ordered=1)):
                for x in (a.B, a.B + 4, a.B + 4 * 37, a.B - 4 * 30):
                    assert call(D, a.B, 5, x, 4, 3, cfg) == E.INVALID_ARGUMENT
        out = spmv.SpTRSVResult(error_code=7, num_levels=9)
        assert spmv.lib().spmv_c_sptrsv_csr_multi(A, ctypes.c_void_p(a.B), 4, None, 4, 4, None,
                                                  ctypes.byref(out)) == E.INVALID_ARGUMENT
        assert out.error_code == E.INVALID_ARGUMENT and out.num_levels == 0
        assert spmv.lib().spmv_c_sptrsv_csr_multi(A, ctypes.c_void_p(a.B), 4, ctypes.c_void_p(a.X), 4, 4, None,
                                                  None) == E.INVALID_FORMAT                    # out may be NULL
    finally:
        for M in (A, R, Z, D):
            spmv.csr_destroy(M)


def _c_cg(spmv, A, F, B, ldb, X, ldx, k, cfg, results):
    return spmv.lib().spmv_c_cg_solve_multi_ic(A, F, ctypes.c_void_p(B), ldb, ctypes.c_void_p(X), ldx, k,
                                               ctypes.byref(cfg) if cfg is not None else None, results)


def test_cg_solve_multi_ic_checks_in_the_stated_order_through_the_c_abi(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    A, R, Z, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), spmv.csr_create(0, 0, 0), _device_header(spmv)
    F = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_L)
    S9 = spmv.csr_wrap_device(9, 9, 16, FAKE_RP, FAKE_CI, FAKE_L)
    try:
        def call(M, Fm, B, ldb, X, ldx, k, cfg, results, written):
            rc = _c_cg(spmv, M, Fm, B, ldb, X, ldx, k, cfg, results)
            a.assert_untouched(written if results is not None else 0, rc)
            for r in a.results:
                r.error_code = 12345
            return rc

        # cg_solve_multi's checks first, in its order, whatever the factor is
        for Fm in (None, F, R):
            for k in (0, 4, K_MAX + 1):
                written = k if 1 <= k <= K_MAX else 0
                assert call(None, Fm, a.B, 1, a.X, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
                assert call(R, Fm, None, 1, a.X, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
                assert call(R, Fm, a.B, 1, None, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
                assert call(R, Fm, a.B, 1, a.X, 1, k, bad_cfg, None, 0) == E.INVALID_ARGUMENT
            for k in (0, -1, K_MAX + 1, 1 << 20):
                assert call(R, Fm, a.B, 40, a.X, 40, k, bad_cfg, a.results, 0) == E.INVALID_ARGUMENT
            assert call(R, Fm, a.B, 3, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
            assert call(R, Fm, a.B, 4, a.X, 3, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
            assert call(R, Fm, a.B, 4, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_DIMENSION
            assert call(A, Fm, a.B, 4, a.X, 4, 4, bad_cfg, a.results, 4) == E.INVALID_FORMAT
            for cfg in (spmv.CGConfig(tolerance=-1e-3), spmv.CGConfig(tolerance=float("nan")),
                        spmv.CGConfig(max_iterations=-1), spmv.CGConfig(engine=1), spmv.CGConfig(engine=2),
                        spmv.CGConfig(engine=-2)):
                assert call(D, Fm, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
            for x in (a.B, a.B + 4, a.B + 4 * 37, a.B - 4 * 30):
                assert call(D, Fm, a.B, 5, x, 4, 3, None, a.results, 3) == E.INVALID_ARGUMENT
        # the empty system comes before the factor
        assert _c_cg(spmv, Z, None, a.B, 4, a.B, 4, 4, bad_cfg, a.results) == E.SUCCESS
        assert [(r.error_code, r.iterations, r.converged) for r in a.results[:4]] == [(0, 0, 1)] * 4
        assert np.all(a.store == POISON)
        a = Arrays(spmv)
        # then the factor: null, its dimensions, its arrays; the preconditioner is not read
        for cfg in (None, spmv.CGConfig(preconditioner=2), spmv.CGConfig(engine=-1)):
            assert call(D, None, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
            assert call(D, R, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_DIMENSION
            assert call(D, S9, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_DIMENSION
            assert call(D, A, a.B, 4, a.X, 4, 4, cfg, a.results, 4) == E.INVALID_FORMAT
    finally:
        for M in (A, R, Z, D, F, S9):
            spmv.csr_destroy(M)


def test_cg_solve_multi_ic_checks_through_python(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.CGConfig(tolerance=-1.0)
    A, R, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), _device_header(spmv)
    F = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_L)
    try:
        def codes(*args, **kw):
            out = spmv.cg_solve_multi_ic(*args, **kw)
            assert np.all(a.store == POISON)
            assert isinstance(out, list) and len(out) >= 1 and len({r.error_code for r in out}) == 1
            assert all((r.iterations, r.converged, r.breakdown) == (0, 0, 0) for r in out)
            return out[0].error_code, len(out)

        assert codes(None, F, a.B, a.X, 0, config=bad_cfg) == (E.INVALID_ARGUMENT, 1)
        assert codes(R, F, None, a.X, 4, ldb=1, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, F, a.B, a.X, K_MAX + 1, config=bad_cfg) == (E.INVALID_ARGUMENT, K_MAX + 1)
        assert codes(R, F, a.B, a.X, 4, ldx=3, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, F, a.B, a.X, 4, config=bad_cfg) == (E.INVALID_DIMENSION, 4)
        assert codes(A, F, a.B, a.B, 4, config=bad_cfg) == (E.INVALID_FORMAT, 4)
        assert codes(D, F, a.B, a.X, 4, config=spmv.CGConfig(engine=1)) == (E.INVALID_ARGUMENT, 4)
        assert codes(D, F, a.B, a.B + 4 * 37, 3, ldb=5, ldx=4) == (E.INVALID_ARGUMENT, 3)
        assert codes(D, None, a.B, a.X, 4) == (E.INVALID_ARGUMENT, 4)
        assert codes(D, R, a.B, a.X, 4, config=spmv.CGConfig(preconditioner=7)) == (E.INVALID_DIMENSION, 4)
        assert codes(D, A, a.B, a.X, 4) == (E.INVALID_FORMAT, 4)
    finally:
        for M in (A, R, D, F):
            spmv.csr_destroy(M)


# ---- the sanitized caller ------------------------------------------------------------------------------------
def test_host_code_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-sptrsv-multi builds tests/cpp/bin/sptrsv_multi_host_sanitized
    (csrc/sptrsv_host.cpp and tests/cpp/sptrsv_multi_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer
    report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-sptrsv-multi"],
                           capture_output=True, text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "sptrsv_multi_host_sanitized")],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
