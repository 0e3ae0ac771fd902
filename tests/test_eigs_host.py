"""eigs_sym / sym_eig_small (include/spmv/eigs.h) on the host side (no GPU): the exported names, the struct layouts
and defaults, the argument checks that come before any device work, in their documented order, through the C ABI and
the Python wrapper; the host twin of sym_eig_small against numpy.linalg.eigh AND, bit for bit, against the numpy
restatement of its rule (tests/eigs_cases.py jacobi); the restatement of the whole header against fp64 dense
eigenvalues on the shared cases; and csrc/eigs_host.cpp under AddressSanitizer + UBSan through a stand-alone caller.

The bounds are the ones measured with the restatement on the CPU, x 4 (eigs_cases.py's docstring and constants).  For
sym_eig_small, measured over eigs_cases.ORDERS x small_matrices(), relative to max |T_ij|: values 9.4e-14,
max |T S - S Theta| 3.2e-14, max |S^T S - I| 1.8e-14, at most 14 sweeps (the test prints what it measures)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import eigs_cases as ec
from conftest import ROOT


# fake, never-dereferenced device addresses: every call below must return before it touches them
VAL, VEC, RES, V0 = 0x100000, 0x200000, 0x300000, 0x400000
FAKE_RP, FAKE_CI, FAKE_VA = 0x500000, 0x600000, 0x700000


def _host_matrix(spmv, rows=8, cols=8):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, i % cols] = 4.0
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


def test_names_exist_in_the_c_abi_the_library_and_python(spmv):
    for name in ("spmv_c_eigs_sym", "spmv_c_sym_eig_small"):
        assert name in spmv.EXPORTED_SYMBOLS
        assert hasattr(spmv.lib(), name)
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    assert "spmv_c_eigs_sym(" in header and "spmv_c_sym_eig_small(" in header
    assert callable(spmv.eigs_sym) and callable(spmv.sym_eig_small)
    R, C = spmv.EigsResult, spmv.EigsConfig
    assert (R.NONE, R.INVARIANT_SUBSPACE, R.NOT_FINITE) == (0, 1, 2) == (ec.NO_BREAKDOWN, ec.INVARIANT_SUBSPACE,
                                                                        ec.NOT_FINITE)
    assert (spmv.EIGS_NO_BREAKDOWN, spmv.EIGS_INVARIANT_SUBSPACE, spmv.EIGS_NOT_FINITE) == (0, 1, 2)
    assert (C.LARGEST, C.SMALLEST) == (0, 1) == (ec.LARGEST, ec.SMALLEST)
    assert (spmv.EIGS_START_SEED, spmv.EIGS_START_TAG) == (ec.START_SEED, ec.START_TAG) == (0x45494753, 0)


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R = spmv.EigsConfig, spmv.EigsResult
    assert ctypes.sizeof(C) == 24 and ctypes.sizeof(R) == 28
    assert [f for f, _ in C._fields_] == ["num_values", "which", "basis", "tolerance", "max_iterations", "engine"]
    assert [f for f, _ in R._fields_] == ["error_code", "iterations", "restarts", "converged", "breakdown",
                                          "max_residual", "elapsed_ms"]
    assert [getattr(C, f).offset for f, _ in C._fields_] == [0, 4, 8, 12, 16, 20]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20, 24]
    c = C()
    assert (c.num_values, c.which, c.basis, np.float32(c.tolerance), c.max_iterations, c.engine) == \
        (1, 0, 0, np.float32(1e-5), 1000, -1)
    r = R()
    assert (r.error_code, r.iterations, r.restarts, r.converged, r.breakdown) == (0, 0, 0, 0, 0)
    assert ec.default_basis(1, 10 ** 6) == 20 and ec.default_basis(12, 10 ** 6) == 24
    assert ec.default_basis(32, 10 ** 6) == 64 and ec.default_basis(3, 5) == 5


def _c_call(spmv, A, values, vectors, ldv, residuals, v0, cfg):
    out = spmv.EigsResult(error_code=12345)
    rc = spmv.lib().spmv_c_eigs_sym(A, ctypes.c_void_p(values), ctypes.c_void_p(vectors), ldv,
                                    ctypes.c_void_p(residuals), ctypes.c_void_p(v0),
                                    ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_checks_in_the_stated_order_through_the_c_abi_and_python(spmv):
    E = spmv.SpMVError
    Cfg = spmv.EigsConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, va, ve, ldv, re, v0, cfg=None: _c_call(spmv, A, va, ve, ldv, re, v0, cfg),
                 lambda A, va, ve, ldv, re, v0, cfg=None: spmv.eigs_sym(A, va, ve, ldv, re, v0, cfg)):
        A = _host_matrix(spmv)
        # 1. nulls, before everything else; the residuals and the start vector may be null
        assert call(None, VAL, VEC, 8, RES, V0, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, None, VEC, 8, RES, V0, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, VAL, None, 8, RES, V0, bad_cfg).error_code == E.INVALID_ARGUMENT
        # 2. not square, before the empty and format checks
        for rows, cols in ((0, 3), (5, 4)):
            R = spmv.csr_create(rows, cols, 0)
            assert call(R, VAL, VEC, 8, None, None, bad_cfg).error_code == E.INVALID_DIMENSION
            spmv.csr_destroy(R)
        # 3. no rows: SUCCESS and nothing written, whatever the config, the pitch and the overlaps
        Z = spmv.csr_create(0, 0, 0)
        res = call(Z, VAL, VAL, -5, VAL, VAL, bad_cfg)
        assert (res.error_code, res.converged, res.iterations, res.restarts, res.breakdown) == (E.SUCCESS, 0, 0, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (a host-only matrix), before the config
        assert call(A, VAL, VEC, 8, None, None, bad_cfg).error_code == E.INVALID_FORMAT
        for rp, ci, va in ((FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
            D = spmv.csr_wrap_device(8, 8, 16, rp, ci, va)
            assert call(D, VAL, VEC, 8, None, None, bad_cfg).error_code == E.INVALID_FORMAT
            spmv.csr_destroy(D)
        D = spmv.csr_wrap_device(100, 100, 300, FAKE_RP, FAKE_CI, FAKE_VA)
        # 5. num_values: 1..32 and <= n; before the basis
        for k in (0, -1, 33, 101):
            assert call(D, VAL, VEC, 100, None, None, Cfg(num_values=k)).error_code == E.INVALID_ARGUMENT
        S5 = spmv.csr_wrap_device(5, 5, 5, FAKE_RP, FAKE_CI, FAKE_VA)
        assert call(S5, VAL, VEC, 5, None, None, Cfg(num_values=6)).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(S5)
        # 6. basis: 0 or k < m <= 64; 7. tolerance; 8. max_iterations; 9. which and engine; 10. ldv.  Each with an
        # overlap present as well: the config comes first
        for cfg in (Cfg(num_values=4, basis=4), Cfg(num_values=4, basis=1), Cfg(num_values=4, basis=-1),
                    Cfg(num_values=4, basis=65), Cfg(tolerance=-1e-3), Cfg(tolerance=float("nan")),
                    Cfg(max_iterations=-1), Cfg(which=2), Cfg(which=-1), Cfg(engine=2), Cfg(engine=-2)):
            assert call(D, VAL, VEC, 100, RES, V0, cfg).error_code == E.INVALID_ARGUMENT
            assert call(D, VAL, VAL, 100, VAL, VAL, cfg).error_code == E.INVALID_ARGUMENT
        assert call(D, VAL, VEC, 99, RES, V0).error_code == E.INVALID_ARGUMENT
        assert call(D, VAL, VEC, -1, RES, V0, Cfg(num_values=3)).error_code == E.INVALID_ARGUMENT
        # 11. overlaps: k = 3, n = 100, ldv = 110: the vectors span 2 * 110 + 100 = 320 floats
        k3 = Cfg(num_values=3, basis=64, engine=0)
        for va, ve, re, v0 in ((VAL, VEC, VAL + 8, V0), (VEC + 4 * 319, VEC, RES, V0), (VAL, VEC, VEC - 8, V0),
                               (VAL, VEC, RES, VEC + 4 * 319), (VAL, VEC, RES, VAL - 4 * 99), (VAL, VEC, RES, RES + 8),
                               (VEC - 8, VEC, None, None), (VAL, VEC, None, VEC)):
            assert call(D, va, ve, 110, re, v0, k3).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_sym_eig_small_checks(spmv):
    E = spmv.SpMVError
    call = spmv.lib().spmv_c_sym_eig_small
    T = np.eye(3)
    values, vectors = np.full(3, -7.0), np.full((3, 3), -7.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for on_device in (0, 1):                    # the checks come before the device is looked at
        assert call(3, None, 3, p(values), p(vectors), on_device) == E.INVALID_ARGUMENT
        assert call(3, p(T), 3, None, p(vectors), on_device) == E.INVALID_ARGUMENT
        assert call(3, p(T), 3, p(values), None, on_device) == E.INVALID_ARGUMENT
        assert call(-1, p(T), 3, p(values), p(vectors), on_device) == E.INVALID_ARGUMENT
        assert call(65, p(T), 65, p(values), p(vectors), on_device) == E.INVALID_ARGUMENT
        assert call(3, p(T), 2, p(values), p(vectors), on_device) == E.INVALID_ARGUMENT
        assert call(0, p(T), 0, p(values), p(vectors), on_device) == E.SUCCESS
    assert np.all(values == -7.0) and np.all(vectors == -7.0)


@pytest.mark.parametrize("n", ec.ORDERS)
def test_host_sym_eig_small_against_eigh_and_the_restatement(spmv, n):
    for name, T in ec.small_matrices(n).items():
        status, values, vectors = spmv.sym_eig_small(T)
        assert status == 0
        scale = max(float(np.max(np.abs(T))), 0.0) or 1.0
        want = np.linalg.eigvalsh(T)
        S = vectors.T                                   # eigenvectors in columns
        figures = (np.max(np.abs(values - want)) / scale, np.max(np.abs(T @ S - S * values)) / scale,
                   np.max(np.abs(S.T @ S - np.eye(n))))
        print(n, name, "values %.2e residual %.2e orthogonality %.2e" % figures)
        assert np.all(np.diff(values) >= 0)
        assert figures[0] <= ec.SMALL_VALUE_BOUND and figures[1] <= ec.SMALL_RESIDUAL_BOUND
        assert figures[2] <= ec.SMALL_ORTHO_BOUND
        # the restatement of the same rule, operation for operation: the same bits
        r_values, r_vectors, sweeps = ec.jacobi(T)
        assert sweeps < ec.MAX_SWEEPS
        assert np.array_equal(values.view(np.uint64), r_values.view(np.uint64)), (n, name)
        assert np.array_equal(vectors.view(np.uint64), r_vectors.view(np.uint64)), (n, name)


def test_host_sym_eig_small_reads_the_leading_dimension(spmv):
    n, ld = 9, 13
    T = ec.small_matrices(n)["random"]
    padded = np.full((n, ld), 7e77)
    padded[:, :n] = T
    values, vectors = np.zeros(n), np.full((n, ld), -3.0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert spmv.lib().spmv_c_sym_eig_small(n, p(padded), ld, p(values), p(vectors), 0) == 0
    _, want_values, want_vectors = spmv.sym_eig_small(T)
    assert np.array_equal(values, want_values) and np.array_equal(vectors[:, :n], want_vectors)
    assert np.all(vectors[:, n:] == -3.0)


def test_the_default_start_vector_is_the_generators(spmv):
    v = ec.default_start(1000)
    assert v.dtype == np.float32 and np.all(np.abs(v) <= 1.0) and np.linalg.norm(v) > 0
    assert np.unique(v).size > 900                      # nothing like the all-ones vector
    assert np.array_equal(v[:17], ec.default_start(17))


CASE_PARAMS = [(name, k, m, which) for name in ec.CASES for k, m in ec.SHAPES for which in (ec.LARGEST, ec.SMALLEST)]


@pytest.mark.parametrize("name,k,m,which", CASE_PARAMS)
def test_restatement_against_fp64(name, k, m, which):
    (n, rp, ci, va), D, lam, Q = ec.dense(name)
    lmax = float(np.max(np.abs(lam)))
    if name in ec.SIMPLE_SPECTRA:                        # only then are the k extreme values themselves demanded
        assert ec.extreme_gap(lam, k, which) >= ec.MIN_RELATIVE_GAP
    out = ec.restate(n, rp, ci, va, k, which, m, tol=ec.TOLERANCE, max_iter=ec.MAX_ITERATIONS)
    values = out["values"].astype(np.float64)
    assert out["converged"] == k and out["found"] == k and out["breakdown"] == ec.NO_BREAKDOWN
    strict = name in ec.SIMPLE_SPECTRA                    # two copies of a multiple eigenvalue may be equal in fp32
    down, up = (np.less, np.greater) if strict else (np.less_equal, np.greater_equal)
    assert np.all(down(np.diff(values), 0)) if which == ec.LARGEST else np.all(up(np.diff(values), 0))
    if name in ec.SIMPLE_SPECTRA:
        error = np.max(np.abs(values - ec.wanted(lam, k, which))) / lmax
    else:                                                # a degenerate spectrum: next to SOME eigenvalue each
        error = max(np.min(np.abs(lam - v)) for v in values) / lmax
    Y = out["vectors"].astype(np.float64)
    ortho = np.max(np.abs(Y @ Y.T - np.eye(k)))
    true = ec.fp64_residuals(D, out["values"], out["vectors"])
    print(name, k, m, which, "steps", out["iterations"], "restarts", out["restarts"], "value %.2e" % error,
          "ortho %.2e" % ortho, "residual %.2e" % (out["max_residual"] / lmax))
    assert error <= ec.VALUE_BOUND and ortho <= ec.ortho_bound(k, m)
    assert out["max_residual"] <= ec.TOLERANCE * lmax * (1 + 1e-6)
    for i in range(k):                                   # the recomputed residuals are honest
        bound = ec.residual_rounding_bound(rp, ci, va, out["values"][i], out["vectors"][i])
        assert abs(true[i] - out["residuals"][i]) <= bound + 2.0 ** -23 * true[i]
    # what the GPU tier compares against is what this run gives
    with open(os.path.join(ROOT, "tests", "golden", ec.GOLDEN)) as f:
        recorded = json.load(f)[ec.golden_key(name, k, m, which)]
    assert abs(recorded["iterations"] - out["iterations"]) <= ec.iteration_spread(k, m)
    if name in ec.SIMPLE_SPECTRA:
        assert abs(recorded["max_residual"] - out["max_residual"] / lmax) <= ec.RESIDUAL_SPREAD


def test_restatement_edges():
    # the identity: invariant after one step, one pair of three
    n = 10
    rp, ci, va = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32)
    out = ec.restate(n, rp, ci, va, 3)
    assert (out["breakdown"], out["iterations"], out["found"], out["converged"]) == (ec.INVARIANT_SUBSPACE, 1, 1, 1)
    assert abs(out["values"][0] - 1) <= 1e-6 and np.all(np.isnan(out["values"][1:]))
    assert np.all(out["vectors"][1:] == 0)
    # a diagonal matrix with distinct entries, n <= m: the whole space, every pair exact to fp32
    d = np.array([3.0, -1.0, 0.5, 7.0, 2.0], np.float32)
    out = ec.restate(5, np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32), d, 3, ec.SMALLEST)
    assert out["converged"] == 3 and out["iterations"] == 5 and out["breakdown"] == ec.NO_BREAKDOWN
    assert np.max(np.abs(out["values"] - np.array([-1.0, 0.5, 2.0]))) <= 4e-6
    # the budget
    n, rp, ci, va = ec.CASES["random_500"]()
    for cap in (0, 1, 7, 8, 9):
        out = ec.restate(n, rp, ci, va, 2, m=8, max_iter=cap)
        assert out["iterations"] == cap and out["found"] == min(2, cap)
    # a NaN in A
    bad = va.copy()
    bad[3] = np.nan
    out = ec.restate(n, rp, ci, bad, 2)
    assert out["breakdown"] == ec.NOT_FINITE and out["converged"] == 0 and np.all(np.isnan(out["values"]))


def test_eigs_host_under_sanitizers():
    """make -C gpu-spmv_amd sanitize-eigs builds tests/cpp/bin/eigs_host_sanitized (csrc/eigs_host.cpp and
    tests/cpp/eigs_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-eigs"], capture_output=True,
                           text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "eigs_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
