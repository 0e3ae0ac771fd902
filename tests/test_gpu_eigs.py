"""eigs_sym / sym_eig_small (include/spmv/eigs.h) on the device.

sym_eig_small's device kernel is held to the host twin bit for bit.  eigs_sym is compared with fp64 dense eigenvalues
and with the recorded runs of the numpy restatement (tests/eigs_cases.py, tests/golden/eigs_restate.json) inside the
bounds measured with that restatement on the CPU, x 4: nothing here is taken from the device's own output.  The
recomputed residuals are held to the fp64 residual of the returned pair within the rounding of one SpMV
(eigs_cases.residual_rounding_bound)."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import eigs_cases as ec
from conftest import ROOT

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
TILED_SMALL = "min_cols=1,min_nnz=1"
SENTINEL = av.SENTINEL
LARGEST, SMALLEST = ec.LARGEST, ec.SMALLEST


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class Problem:
    """A matrix on the device (csr_from_arrays + csr_to_gpu)."""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0

    def run(self, k, which=LARGEST, m=0, ldv=None, offset=0, v0=None, residuals=True, A=None, **cfg):
        """(result, values, vectors k x n, residuals); every output array is a sentinel-filled buffer whose every
        element outside the documented ranges must come back unchanged"""
        gpu, n = self.gpu, self.n
        ldv = n if ldv is None else ldv
        total = offset + k * ldv + 8
        d_vec = gpu.CudaBuffer(total, "uint32")
        d_val = gpu.CudaBuffer(k + 8, "uint32")
        d_res = gpu.CudaBuffer(k + 8, "uint32")
        d_vec.copyFromHost(np.full(total, SENTINEL, np.uint32), total)
        d_val.copyFromHost(np.full(k + 8, SENTINEL, np.uint32), k + 8)
        d_res.copyFromHost(np.full(k + 8, SENTINEL, np.uint32), k + 8)
        d_v0 = None
        if v0 is not None:
            d_v0 = gpu.CudaBuffer(n)
            d_v0.copyFromHost(np.asarray(v0, np.float32), n)
        config = gpu.EigsConfig(num_values=k, which=which, basis=m, **cfg)
        res = gpu.eigs_sym(self.A if A is None else A, d_val.get(), d_vec.get() + 4 * offset, ldv,
                           d_res.get() if residuals else None, d_v0.get() if d_v0 is not None else None, config)
        raw = d_vec.copyToHost(total)
        keep = np.ones(total, bool)
        for i in range(k):
            keep[offset + i * ldv: offset + i * ldv + n] = False
        assert np.all(raw[keep] == SENTINEL), "padding or guard written"
        val, rsd = d_val.copyToHost(k + 8), d_res.copyToHost(k + 8)
        assert np.all(val[k:] == SENTINEL) and np.all(rsd[k:] == SENTINEL)
        if not residuals:
            assert np.all(rsd == SENTINEL)
        vectors = np.stack([raw[offset + i * ldv: offset + i * ldv + n] for i in range(k)]).view(np.float32)
        for b in (d_vec, d_val, d_res) + ((d_v0,) if d_v0 is not None else ()):
            b.release()
        return res, val[:k].view(np.float32).copy(), vectors, rsd[:k].view(np.float32).copy()

    def true_residuals(self, values, vectors):
        return np.array([np.linalg.norm(spd.spmv64(self.rp, self.ci, self.va, y) - float(t) * y.astype(np.float64))
                         for t, y in zip(values, vectors)])

    def check_honest(self, values, vectors, residuals):
        true = self.true_residuals(values, vectors)
        for i in range(len(values)):
            bound = ec.residual_rounding_bound(self.rp, self.ci, self.va, values[i], vectors[i])
            print("pair", i, "reported", residuals[i], "true", true[i], "bound", bound)
            assert abs(true[i] - residuals[i]) <= bound + 2.0 ** -23 * true[i], (i, residuals[i], true[i], bound)
        return true

    def close(self):
        self.gpu.csr_destroy(self.A)


_problems = {}


@pytest.fixture(scope="module")
def problems(gpu):
    def get(name):
        if name not in _problems:
            _problems[name] = Problem(gpu, *ec.dense(name)[0])
        return _problems[name]
    yield get
    for p in _problems.values():
        p.close()
    _problems.clear()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", ec.GOLDEN)) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------ 1. sym_eig_small, bit for bit
@pytest.mark.parametrize("n", ec.ORDERS)
def test_sym_eig_small_on_the_device_equals_the_host_twin(gpu, n):
    for name, T in ec.small_matrices(n).items():
        h_status, h_values, h_vectors = gpu.sym_eig_small(T)
        d_status, d_values, d_vectors = gpu.sym_eig_small(T, on_device=True)
        assert h_status == 0 and d_status == 0
        assert np.array_equal(h_values.view(np.uint64), d_values.view(np.uint64)), (n, name)
        assert np.array_equal(h_vectors.view(np.uint64), d_vectors.view(np.uint64)), (n, name)


# ------------------------------------------------------------------------------------ 2. against fp64 eigenvalues
CASE_PARAMS = [(name, k, m, which) for name in ec.CASES for k, m in ec.SHAPES for which in (LARGEST, SMALLEST)]


@pytest.mark.parametrize("name,k,m,which", CASE_PARAMS)
def test_eigs_sym_against_fp64(gpu, problems, recorded, name, k, m, which):
    (n, rp, ci, va), D, lam, Q = ec.dense(name)
    lmax = float(np.max(np.abs(lam)))
    p = problems(name)
    res, values, vectors, residuals = p.run(k, which, m, tolerance=ec.TOLERANCE, max_iterations=ec.MAX_ITERATIONS,
                                            engine=0)
    v64 = values.astype(np.float64)
    if name in ec.SIMPLE_SPECTRA:
        assert ec.extreme_gap(lam, k, which) >= ec.MIN_RELATIVE_GAP
        error = np.max(np.abs(v64 - ec.wanted(lam, k, which))) / lmax
    else:
        error = max(np.min(np.abs(lam - v)) for v in v64) / lmax
    Y = vectors.astype(np.float64)
    ortho = np.max(np.abs(Y @ Y.T - np.eye(k)))
    want = recorded[ec.golden_key(name, k, m, which)]
    print(name, k, m, which, "steps", res.iterations, "recorded", want["iterations"], "restarts", res.restarts,
          "value %.2e ortho %.2e max residual %.2e (recorded %.2e)" % (error, ortho, res.max_residual / lmax,
                                                                        want["max_residual"]))
    assert (res.error_code, res.breakdown) == (0, 0)
    assert res.converged == k
    strict = name in ec.SIMPLE_SPECTRA                    # two copies of a multiple eigenvalue may be equal in fp32
    down, up = (np.less, np.greater) if strict else (np.less_equal, np.greater_equal)
    assert np.all(down(np.diff(v64), 0)) if which == LARGEST else np.all(up(np.diff(v64), 0))
    assert error <= ec.VALUE_BOUND
    assert ortho <= ec.ortho_bound(k, m)
    true = p.check_honest(values, vectors, residuals)
    assert res.max_residual == residuals.max()
    assert np.all(residuals.astype(np.float64) <= np.float64(np.float32(ec.TOLERANCE)) * lmax * (1 + 1e-6))
    assert np.all(true <= ec.TOLERANCE * lmax * (1 + 1e-6) +
                  np.array([ec.residual_rounding_bound(rp, ci, va, values[i], vectors[i]) for i in range(k)]))
    assert abs(res.iterations - want["iterations"]) <= ec.iteration_bound(name, k, m)
    if name in ec.SIMPLE_SPECTRA:
        assert abs(res.max_residual / lmax - want["max_residual"]) <= ec.RESIDUAL_SPREAD


# ------------------------------------------------------------------------------------ 3. edges of the kernels
def edge_system(n):
    if n == 1:
        return 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.5], np.float32)
    return spd.random_spd(n, min(7, n - 1), seed=100 + n)


def check_pairs(p, res, values, vectors, residuals, k, which, ortho=ec.ORTHO_BOUND):
    """what holds without a dense decomposition: every pair returned, ordered, orthonormal, with an honest residual"""
    assert (res.error_code, res.converged) == (0, k), (res.error_code, res.converged, res.breakdown, res.iterations)
    v64 = values.astype(np.float64)
    assert np.all(np.diff(v64) <= 0) if which == LARGEST else np.all(np.diff(v64) >= 0)
    Y = vectors.astype(np.float64)
    assert np.max(np.abs(Y @ Y.T - np.eye(k))) <= ortho
    p.check_honest(values, vectors, residuals)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_edges_of_the_basis_walk(gpu, n):
    system = edge_system(n)
    p = Problem(gpu, *system)
    try:
        lam = np.linalg.eigvalsh(ec_dense(system)) if n <= 1100 else None
        for k in sorted({1, min(3, n)}):
            for ldv, offset in ((n, 0), (n + 3, 1)):
                res, values, vectors, residuals = p.run(k, LARGEST, ldv=ldv, offset=offset, engine=0)
                check_pairs(p, res, values, vectors, residuals, k, LARGEST)
                if lam is not None:
                    assert np.max(np.abs(values - lam[::-1][:k])) <= ec.VALUE_BOUND * np.max(np.abs(lam))
                else:
                    assert np.all(residuals <= 1e-5 * abs(values[0]) * (1 + 1e-3))
    finally:
        p.close()


def ec_dense(system):
    n, rp, ci, va = system
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64))), ci), va.astype(np.float64))
    return D


@pytest.mark.parametrize("k,m", [(2, 8), (2, 9), (2, 16), (2, 17), (2, 64), (32, 64), (31, 32)])
def test_group_of_eight_boundaries_of_the_basis(gpu, problems, k, m):
    (n, rp, ci, va), D, lam, Q = ec.dense("random_500")
    p = problems("random_500")
    res, values, vectors, residuals = p.run(k, LARGEST, m, engine=0, max_iterations=ec.MAX_ITERATIONS)
    # one new column per cycle, as at (7, 9): the orthogonality figure of that shape
    check_pairs(p, res, values, vectors, residuals, k, LARGEST,
                ec.ORTHO_BOUND_7_9 if ec.iteration_spread(k, m) == 1 else ec.ORTHO_BOUND)
    assert np.max(np.abs(values - lam[::-1][:k])) <= ec.VALUE_BOUND * np.max(np.abs(lam))


def test_diagonal_matrix_identity_and_an_eigenvector_start(gpu):
    # distinct diagonal entries, n <= m: the whole space after n steps, every pair exact to fp32
    n = 12
    d = (np.arange(n, dtype=np.float32) * np.float32(0.75) - np.float32(3.0))[::-1].copy()
    idx = np.arange(n, dtype=np.int32)
    p = Problem(gpu, n, np.arange(n + 1, dtype=np.int32), idx, d)
    for which, want in ((LARGEST, np.sort(d)[::-1][:4]), (SMALLEST, np.sort(d)[:4])):
        res, values, vectors, residuals = p.run(4, which, engine=0)
        check_pairs(p, res, values, vectors, residuals, 4, which)
        assert res.iterations == n and res.restarts == 0 and res.breakdown == 0
        assert np.max(np.abs(values - want)) <= ec.VALUE_BOUND * np.max(np.abs(d))
        for i in range(4):                       # y_i = +- e_j
            j = int(np.argmax(np.abs(vectors[i])))
            assert d[j] == want[i] and abs(abs(vectors[i][j]) - 1) <= ec.ORTHO_BOUND
    # a start vector that is an eigenvector: invariant after one step; one pair of one, one pair of three
    e3 = np.zeros(n, np.float32)
    e3[3] = 2.0
    res, values, vectors, _ = p.run(1, LARGEST, v0=e3, engine=0)
    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, 1, 1, 0)
    assert values[0] == d[3] and abs(vectors[0][3]) == 1.0
    res, values, vectors, residuals = p.run(3, SMALLEST, v0=e3, engine=0)
    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, 1, 1, gpu.EigsResult.INVARIANT_SUBSPACE)
    assert values[0] == d[3] and np.all(np.isnan(values[1:])) and np.all(np.isnan(residuals[1:]))
    assert np.all(vectors[1:] == 0) and residuals[0] == 0
    # a zero start vector of the caller's: INVALID_ARGUMENT, nothing written (run() checks the sentinels)
    res, values, vectors, _ = p.run(2, LARGEST, v0=np.zeros(n, np.float32), engine=0)
    assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT
    assert np.all(bits(values) == SENTINEL) and np.all(bits(vectors) == SENTINEL)
    p.close()
    # the identity with the default start vector
    n = 300
    p = Problem(gpu, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n, np.float32))
    res, values, vectors, residuals = p.run(3, LARGEST, engine=0)
    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, 1, 1, gpu.EigsResult.INVARIANT_SUBSPACE)
    assert abs(values[0] - 1) <= 1e-6 and np.all(np.isnan(values[1:])) and np.all(vectors[1:] == 0)
    start = ec.default_start(n).astype(np.float64)
    assert np.max(np.abs(np.abs(vectors[0]) - np.abs(start) / np.linalg.norm(start))) <= 1e-6
    p.close()


def test_nan_in_a_is_not_finite_with_defined_outputs(gpu):
    n, rp, ci, va = ec.CASES["random_500"]()
    bad = va.copy()
    bad[11] = np.nan
    p = Problem(gpu, n, rp, ci, bad)
    for engine in (0, 1):
        res, values, vectors, residuals = p.run(3, LARGEST, ldv=n + 2, offset=3, engine=engine)
        assert (res.error_code, res.breakdown, res.converged) == (0, gpu.EigsResult.NOT_FINITE, 0)
        assert np.isnan(res.max_residual) and res.iterations <= 2
        assert np.all(np.isnan(values)) and np.all(np.isnan(residuals)) and np.all(vectors == 0)
    nan_start = np.ones(n, np.float32)
    nan_start[5] = np.inf
    res, values, vectors, _ = p.run(2, LARGEST, v0=nan_start, engine=0)
    assert (res.error_code, res.breakdown, res.iterations) == (0, gpu.EigsResult.NOT_FINITE, 0)
    assert np.all(np.isnan(values)) and np.all(vectors == 0)
    p.close()


# ------------------------------------------------------------------------------------ 4. the budget
@pytest.mark.parametrize("cap", [0, 1, 7, 8, 9])
def test_budget(gpu, problems, cap):
    m, k = 8, 2
    (n, rp, ci, va), D, lam, Q = ec.dense("random_500")
    p = problems("random_500")
    res, values, vectors, residuals = p.run(k, LARGEST, m, max_iterations=cap, engine=0, tolerance=1e-7)
    found = min(k, cap)
    assert res.error_code == 0 and res.iterations == cap and res.breakdown == 0
    assert res.restarts == (1 if cap > m else 0)
    assert np.all(np.isnan(values[found:])) and np.all(vectors[found:] == 0)
    if found:
        # the pairs are the Ritz pairs of the Krylov space of `cap` steps: compare with the restatement's
        want = ec.restate(n, rp, ci, va, k, LARGEST, m, tol=1e-7, max_iter=cap)
        assert want["iterations"] == cap and want["restarts"] == res.restarts
        assert np.max(np.abs(values[:found] - want["values"][:found])) <= ec.VALUE_BOUND * np.max(np.abs(lam))
        p.check_honest(values[:found], vectors[:found], residuals[:found])
        assert want["converged"] == 0 and res.converged == 0      # nine steps are far from 1e-7
    else:
        assert res.converged == 0 and res.max_residual == 0


# ------------------------------------------------------------------------------------ 5. the same bits on two runs
def test_two_runs_give_the_same_bits_and_the_engines_agree(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)               # lets the tiled engine take a small matrix
    system = spd.random_spd(3000, 7, seed=9)
    p = Problem(gpu, *system)
    try:
        runs = {}
        for engine in (0, 1):
            a = p.run(4, SMALLEST, 20, engine=engine)
            b = p.run(4, SMALLEST, 20, engine=engine)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(bits(x), bits(y)), engine
            assert (a[0].iterations, a[0].restarts, a[0].converged) == (b[0].iterations, b[0].restarts, 4)
            runs[engine] = a
        assert gpu.csr_has_tiled_plan(p.A)
        n, rp, ci, va = system                                 # Gershgorin: max |lambda| <= the largest absolute row sum
        lmax = float(np.max(np.bincount(np.repeat(np.arange(n), np.diff(rp)), weights=np.abs(va).astype(np.float64))))
        r0, r1 = runs[0], runs[1]
        assert np.max(np.abs(r0[1] - r1[1])) <= 4 * 1.3e-7 * lmax
        assert abs(r0[0].iterations - r1[0].iterations) <= 4 * ec.iteration_spread(4, 20)
        check_pairs(p, *r1, 4, SMALLEST)
        # auto on a matrix that already holds a plan: the tiled engine from the first step, the same bits as engine 1
        auto = p.run(4, SMALLEST, 20, engine=-1)
        for x, y in zip(auto[1:], r1[1:]):
            assert np.array_equal(bits(x), bits(y))
        assert auto[0].iterations == r1[0].iterations
    finally:
        p.close()


# ------------------------------------------------------------------------------------ 6. views
def test_matrix_arrays_as_views_into_larger_buffers(gpu):
    n, rp, ci, va = spd.random_spd(289, 5, seed=4)
    p = Problem(gpu, n, rp, ci, va)
    try:
        plain = p.run(3, LARGEST, 16, engine=0)
        bare = p.run(3, LARGEST, 16, engine=0, residuals=False)         # d_residuals may be null
        assert bare[0].converged == 3 and np.array_equal(bits(bare[1]), bits(plain[1]))
        assert bare[0].max_residual == plain[0].max_residual
        with av.Views(gpu) as views:
            A, _ = views.csr(n, n, rp, ci, va, (1, 2, 3))
            viewed = p.run(3, LARGEST, 16, ldv=n + 1, offset=1, engine=0, A=A)
            assert (viewed[0].error_code, viewed[0].iterations, viewed[0].converged) == (0, plain[0].iterations, 3)
            for x, y in zip(viewed[1:], plain[1:]):
                assert np.array_equal(bits(x), bits(y))
            views.check_guards("eigs_sym")
    finally:
        p.close()


# ------------------------------------------------------------------------------------ 7. the C++ caller
def test_cpp_eigs_smoke_agrees_with_python(gpu):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "eigs_smoke")
    assert os.path.exists(exe), "build() compiles tests/cpp/eigs_smoke.cpp"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    printed = {}
    for line in run.stdout.splitlines():
        f = line.split()
        if len(f) >= 5 and f[0] == "which" and f[2] == "value":
            printed[(int(f[1]), int(f[3]))] = np.float32(f[4])
    assert len(printed) == 8
    rows, cols = 24, 20                                  # the matrix of eigs_smoke.cpp, value for value
    n = rows * cols
    rp, ci, va = [0], [], []
    for i in range(rows):
        for j in range(cols):
            row = i * cols + j
            if i > 0: ci.append(row - cols); va.append(np.float32(-1))
            if j > 0: ci.append(row - 1); va.append(np.float32(-1))
            ci.append(row)
            va.append(np.float32(4) + np.float32(0.01) * np.float32(row) / np.float32(n))
            if j + 1 < cols: ci.append(row + 1); va.append(np.float32(-1))
            if i + 1 < rows: ci.append(row + cols); va.append(np.float32(-1))
            rp.append(len(ci))
    p = Problem(gpu, n, np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, np.float32))
    try:
        for which in (LARGEST, SMALLEST):
            res, values, _, _ = p.run(4, which, ldv=n + 5, engine=0)
            assert res.converged == 4
            for i in range(4):
                assert bits(values[i]) == bits(printed[(which, i)]), (which, i, values[i], printed[(which, i)])
    finally:
        p.close()
