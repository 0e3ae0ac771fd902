"""cg_solve_multi_ic (include/spmv/cg.h) on the device.

The contract is bitwise: column j of the batched solve is cg_solve_ic(engine = 0) on that column alone.  So the
reference in every comparison is cg_solve_ic itself, and x, iterations, converged, breakdown, error_code and the bits
of relative_residual are compared at zero tolerance, whatever the other columns do.  Covered: the matrices of
tests/test_gpu_cg_ic.py with their IC(0) factors at every window shape; every lane count of A's SpMV (the systems of
tests/exact_data.py, preconditioned by the factor of their canonical form); columns that finish at different steps;
per-column breakdown; an exact factor; steps after `done`; the layouts; reproducibility; the rejections with X
untouched; and isolation from A's caches."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import ic0_cases as cases
from array_views import SENTINEL, View

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
assert_bits = importlib.import_module("test_gpu_lane_sweep").assert_bits

POISON = SENTINEL.view(np.float32)
ALL_K = (1, 2, 3, 4, 5, 8, 9, 16, 32)
SOME_K = (3, 8, 9)
TOL = 1e-6

MATRICES = {                                     # tests/test_gpu_cg_ic.py MATRICES
    "poisson2d(16)": lambda: spd.poisson2d(16),
    "poisson2d(24)": lambda: spd.poisson2d(24),
    "poisson3d(8)": lambda: spd.poisson3d(8),
}
FULL_K_NAME = "poisson2d(24)"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Device:
    """A matrix and a factor on the device, cg_solve_ic on one column as the reference and cg_solve_multi_ic in any
    layout.  factor: (rp, ci, va) of the matrix whose IC(0) factor preconditions (its own pattern; default A itself)."""

    def __init__(self, gpu, n, rp, ci, va, factor=None):
        self.gpu, self.n, self.rp = gpu, n, rp
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        f_rp, f_ci, f_va = (rp, ci, va) if factor is None else factor
        self.M = gpu.csr_from_arrays(n, n, f_rp, f_ci, f_va)
        assert gpu.csr_to_gpu(self.M) == 0
        self.d_l = gpu.CudaBuffer(f_ci.size)
        res = gpu.ic0_csr(self.M, self.d_l)
        assert res.error_code == 0 and res.bad_pivot == -1, (res.error_code, res.bad_pivot)
        self.F = gpu.csr_wrap_device(n, n, int(f_ci.size), self.M.contents.d_row_ptrs, self.M.contents.d_col_indices,
                                     self.d_l.get())
        self.d_b, self.d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        self._single = {}

    def single(self, b, x0, key=None, F=None, **cfg):
        """(result, x) of cg_solve_ic(engine = 0) on one column; kept under `key` when one is given."""
        if key is not None and key in self._single:
            return self._single[key]
        self.d_b.copyFromHost(np.asarray(b, np.float32), self.n)
        self.d_x.copyFromHost(np.asarray(x0, np.float32), self.n)
        res = self.gpu.cg_solve_ic(self.A, self.F if F is None else F, self.d_b, self.d_x,
                                   self.gpu.CGConfig(engine=0, **cfg))
        out = (res, self.d_x.copyToHost(self.n))
        if key is not None:
            self._single[key] = out
        return out

    def multi(self, B, X0, ldb=None, ldx=None, offset=0, engine=0, F=None, **cfg):
        """(results, X) of cg_solve_multi_ic on the n x k arrays B and X0, stored with the given leading dimensions in
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
            results = self.gpu.cg_solve_multi_ic(self.A, self.F if F is None else F, vb.ptr, vx.ptr, k, ldb, ldx,
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
        for M in (self.F, self.M, self.A):
            self.gpu.csr_destroy(M)
        for buf in (self.d_l, self.d_b, self.d_x):
            buf.release()


def assert_column(rp, res, x, ref, x_ref, what):
    """One column of the batch against its own cg_solve_ic run, to the bit."""
    got = (res.error_code, res.iterations, res.converged, res.breakdown)
    want = (ref.error_code, ref.iterations, ref.converged, ref.breakdown)
    assert got == want, (what, got, want)
    rel, rel_ref = np.float32(res.relative_residual), np.float32(ref.relative_residual)
    assert rel.view(np.uint32) == rel_ref.view(np.uint32), (what, rel, rel_ref)
    assert_bits(rp, x, x_ref, what)


def assert_parity(dev, B, X0, what, keys=None, layout=None, **cfg):
    """cg_solve_multi_ic on (B, X0) against cg_solve_ic column by column; returns (results, X)."""
    results, X = dev.multi(B, X0, **dict(layout or {}, **cfg))
    assert len(results) == B.shape[1]
    assert len({r.elapsed_ms for r in results}) == 1
    for j in range(B.shape[1]):
        ref, x_ref = dev.single(B[:, j], X0[:, j], key=None if keys is None else keys[j], **cfg)
        assert_column(dev.rp, results[j], X[:, j], ref, x_ref, what + ("column", j))
    return results, X


def columns(n, k, seed=7, first=None):
    """B (n x k): seeded uniform columns (column j the same whatever k), `first` in column 0 when given"""
    B = np.empty((n, k), np.float32)
    for j in range(k):
        B[:, j] = np.random.default_rng([seed, j]).uniform(-64.0, 64.0, n).astype(np.float32)
    if first is not None:
        B[:, 0] = first
    return B


# ------------------------------------------------------------------------------------------ 1. the IC matrices
@pytest.mark.parametrize("name", list(MATRICES))
def test_column_parity_on_the_ic_matrices(gpu, name):
    """cgm_update_kernel<W, true> / cgm_rz_kernel<W> / cgm_direction_kernel<W, true> (W = 4 and 8) and the k-wide
    triangular solves on the windowed workspace with one, two and four windows; F = ic0_csr over A's structure."""
    n, rp, ci, va = MATRICES[name]()
    dev = Device(gpu, n, rp, ci, va)
    try:
        iterations = set()
        for k in (ALL_K if name == FULL_K_NAME else SOME_K):
            B = columns(n, k)
            results, _ = assert_parity(dev, B, np.zeros_like(B), (name, k), keys=list(range(k)), tolerance=TOL)
            assert all(r.error_code == 0 and r.converged and r.iterations > 0 for r in results)
            iterations |= {r.iterations for r in results}
        print(name, "iterations seen", sorted(iterations))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 2. every lane count
def canonical(n, rp, ci, va):
    """the same matrix with strictly ascending columns and repeated entries summed: what ic0_csr accepts"""
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    uniq, inverse = np.unique(r * n + ci, return_inverse=True)
    vals = np.zeros(uniq.size, np.float64)
    np.add.at(vals, inverse, va.astype(np.float64))
    rows = uniq // n
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rp2, (uniq % n).astype(np.int32), vals.astype(np.float32)


# Systems of ed.SOLVER_NAMES that have no IC(0) preconditioner, by name with the reason.  The systems store their rows
# unsorted with repeated entries, which ic0_csr rejects, so the factor is taken from their canonical form (a pattern of
# its own, as cg_solve_ic allows); with that, ic0_cpu_csr factors all fourteen without a bad pivot (checked on the CPU
# when this test was written, and asserted by Device on the device).
LEFT_OUT = {}


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_column_parity_at_every_lane_count_of_the_spmv(gpu, name):
    """cgm_spmv_dot<L, W, NW> and cgm_init_kernel<L, 4, W> at L = 1 ... 64 under the IC loop; the factor's triangles
    get denser with L, so the k-wide triangular solves run at several lane counts of their own."""
    assert 3 * len(LEFT_OUT) <= len(ed.SOLVER_NAMES) and set(LEFT_OUT) <= set(ed.SOLVER_NAMES)
    if name in LEFT_OUT:
        return
    L, n, rp, ci, va, _, b = ed.solver_system(name, symmetric=True)
    dev = Device(gpu, n, rp, ci, va, factor=canonical(n, rp, ci, va))
    try:
        for k in (3, 9):
            B = columns(n, k, first=b)
            cfg = dict(tolerance=TOL, max_iterations=40)
            results, _ = assert_parity(dev, B, np.zeros_like(B), (name, L, k), keys=list(range(k)), **cfg)
            assert all(r.error_code == 0 and r.iterations > 0 for r in results)
            print(name, "L", L, "k", k, "iterations", [r.iterations for r in results])
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. finishing apart
def test_columns_that_finish_at_different_steps(gpu):
    """poisson2d(24), k = 6: a zero column (x = 0 over its guess), a column whose guess already meets the tolerance (0
    iterations, x untouched), b at three scales (2^-20, 1, 2^20: the same steps, other bits) and a loose column that
    max_iterations cuts off; then the same batch with room for every column.  Frozen columns sit in a window with
    running ones throughout, and the triangular solves keep recomputing their z."""
    n, rp, ci, va = spd.poisson2d(24)
    dev = Device(gpu, n, rp, ci, va)
    try:
        rng = np.random.default_rng(21)
        B = np.zeros((n, 6), np.float32)
        X0 = rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32)       # the zero column's guess must be overwritten
        B[:, 1] = rng.uniform(-1.0, 1.0, n)
        solved, x_solved = dev.single(B[:, 1], np.zeros(n), tolerance=1e-6)
        assert solved.converged and solved.iterations > 4
        X0[:, 1] = x_solved
        base = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        B[:, 2], B[:, 3], B[:, 4] = base * np.float32(2.0 ** -20), base, base * np.float32(2.0 ** 20)
        B[:, 5] = rng.uniform(-1.0, 1.0, n)
        X0[:, 2:5] = 0.0
        results, X = assert_parity(dev, B, X0, ("finish", 4), tolerance=1e-4, max_iterations=4)
        its = [r.iterations for r in results]
        print("iterations", its, "converged", [r.converged for r in results])
        assert (its[0], results[0].converged) == (0, 1) and not X[:, 0].any()
        assert (its[1], results[1].converged) == (0, 1) and np.array_equal(bits(X[:, 1]), bits(X0[:, 1]))
        assert (its[5], results[5].converged, results[5].breakdown) == (4, 0, 0)
        results, X = assert_parity(dev, B, X0, ("finish", 1000), tolerance=1e-4, max_iterations=1000)
        assert all(r.converged for r in results) and results[5].iterations > 4
        assert results[2].iterations == results[3].iterations == results[4].iterations
        assert len({r.iterations for r in results}) >= 2
    finally:
        dev.close()


def test_breakdown_is_per_column(gpu):
    """A = diag(P, -P), P = poisson2d(16), preconditioned by the factor of diag(P, P): both are block diagonal, so a
    column that starts in one block stays there.  b in the first block converges; b in the second block is the
    negative-definite case of tests/test_gpu_cg_ic.py (p.q <= 0 at the first step, x stays at its guess); a mixed b
    does what cg_solve_ic does; all in one window with a zero column."""
    m, rp1, ci1, va1 = spd.poisson2d(16)
    n = 2 * m
    rp = np.concatenate([rp1, rp1[1:] + rp1[-1]]).astype(np.int32)
    ci = np.concatenate([ci1, ci1 + m]).astype(np.int32)
    va = np.concatenate([va1, -va1]).astype(np.float32)
    dev = Device(gpu, n, rp, ci, va, factor=(rp, ci, np.concatenate([va1, va1]).astype(np.float32)))
    try:
        rng = np.random.default_rng(4)
        B = np.zeros((n, 5), np.float32)
        B[:m, 0] = rng.uniform(-1.0, 1.0, m)
        B[m:, 1] = rng.uniform(-1.0, 1.0, m)
        B[:, 2] = rng.uniform(-1.0, 1.0, n)
        B[:m, 4] = rng.uniform(-1.0, 1.0, m)
        X0 = np.zeros_like(B)
        X0[:, 1] = 0.25
        X0[:m, 1] = 0.0                                               # the guess stays inside the second block too
        results, X = assert_parity(dev, B, X0, ("breakdown",), tolerance=TOL, max_iterations=200)
        flags = [(r.converged, r.breakdown) for r in results]
        print("iterations", [r.iterations for r in results], "flags", flags)
        assert flags[0] == (1, 0) and flags[4] == (1, 0) and flags[3] == (1, 0)
        assert flags[1] == (0, 1) and results[1].iterations == 0
        assert np.array_equal(bits(X[:, 1]), bits(X0[:, 1])) and np.isfinite(X).all()
        assert results[0].iterations > 1 and not X[:, 3].any()
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 4. exact factor
def test_an_exact_factor_makes_every_column_a_direct_solve(gpu):
    n, rp, ci, va, fact = cases.exact_tridiagonal(257)
    np.testing.assert_array_equal(bits(cases.prove_exact(n, rp, ci, va)), bits(fact))
    dev = Device(gpu, n, rp, ci, va)
    try:
        np.testing.assert_array_equal(bits(dev.d_l.copyToHost(ci.size)), bits(fact))
        for k in (3, 9):
            B = np.stack([np.random.default_rng(seed).uniform(-1.0, 1.0, n) for seed in range(1, k + 1)],
                         axis=1).astype(np.float32)
            results, _ = assert_parity(dev, B, np.zeros_like(B), ("exact factor", k), tolerance=1e-4)
            for r in results:
                assert (r.error_code, r.converged, r.breakdown, r.iterations) == (0, 1, 0, 1)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 5. steps after done
def test_steps_after_done_change_nothing(gpu):
    n, rp, ci, va = spd.poisson2d(24)
    dev = Device(gpu, n, rp, ci, va)
    try:
        B = columns(n, 5, seed=9)
        B[:, 3] *= np.float32(1e-3)
        X0 = np.zeros_like(B)
        full, X_full = assert_parity(dev, B, X0, ("full",), tolerance=TOL)
        last = max(r.iterations for r in full)
        assert all(r.converged for r in full) and last >= 3
        fields = lambda rs: [(r.error_code, r.iterations, r.converged, r.breakdown,
                              int(np.float32(r.relative_residual).view(np.uint32))) for r in rs]
        for extra in (0, 1, 5):                                       # stopped at the last column's count, and past it
            res, X = dev.multi(B, X0, tolerance=TOL, max_iterations=last + extra)
            assert fields(res) == fields(full) and np.array_equal(bits(X), bits(X_full)), extra
        for cut in (1, 2):
            res, _ = assert_parity(dev, B, X0, ("cut", cut), tolerance=TOL, max_iterations=cut)
            assert all((r.iterations, r.converged, r.breakdown) == (cut, 0, 0) for r in res)
        res, X = dev.multi(B, np.full_like(B, 0.5), max_iterations=0)
        assert all((r.error_code, r.iterations, r.converged) == (0, 0, 0) for r in res) and np.all(X == np.float32(0.5))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. layouts
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("ldb,ldx", [(5, 5), (8, 8), (7, 6), (5, 12)])
def test_leading_dimensions_and_alignment(gpu, ldb, ldx, offset):
    """k = 5 in the caller's arrays; the workspace the triangular solves run on is the solver's own whatever the
    layout.  Device.multi asserts the poison in X's padding columns, around both arrays, and B itself."""
    n, rp, ci, va = spd.poisson3d(8)
    dev = Device(gpu, n, rp, ci, va)
    try:
        B = columns(n, 5, seed=3)
        X0 = np.zeros_like(B)
        X0[:, 2] = np.random.default_rng(5).uniform(-1.0, 1.0, n)    # a non-zero guess goes through cgm_init_kernel's walk
        results, _ = assert_parity(dev, B, X0, (ldb, ldx, offset), layout=dict(ldb=ldb, ldx=ldx, offset=offset),
                                   tolerance=TOL)
        assert all(r.converged for r in results)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 7. reproducibility
def test_two_runs_and_a_column_permutation_give_the_same_bits(gpu):
    n, rp, ci, va = spd.poisson2d(24)
    dev = Device(gpu, n, rp, ci, va)
    try:
        k = 11
        rng = np.random.default_rng(3)
        B = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
        B[:, 4] = 0.0
        B[:, 6] *= np.float32(1e-4)
        X0 = rng.uniform(-1.0, 1.0, (n, k)).astype(np.float32)
        cfg = dict(tolerance=1e-5, max_iterations=200)
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


# ------------------------------------------------------------------------------------------ 8. rejections
@pytest.mark.parametrize("case", ["zero", "negative", "nan", "missing"])
def test_a_bad_factor_diagonal_is_rejected_and_x_is_untouched(gpu, case):
    """tests/test_gpu_cg_ic.py's four factors, k = 3, found on the device in the one setup read-back"""
    a_rp, a_ci, a_va = [0, 2, 4, 6, 8], [0, 1, 0, 1, 2, 3, 2, 3], [4, .5, .5, 3, 2, 1, 1, 5]
    if case == "zero":                          # (2,2) stored as 0
        rp, ci, va = a_rp, a_ci, [2, .25, .25, 1.5, 0, 1, 1, 2]
    elif case == "negative":                    # (1,1) < 0
        rp, ci, va = a_rp, a_ci, [2, .25, .25, -1.5, 1, 1, 1, 2]
    elif case == "nan":                         # (2,2) = NaN
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 2, 3], [2, .25, .25, 1.5, np.nan, 2]
    else:                                       # rows 2 and 3 hold only their off-diagonal entries
        rp, ci, va = [0, 2, 4, 5, 6], [0, 1, 0, 1, 3, 2], [2, .25, .25, 1.5, 1, 1]
    i32, f32 = lambda a: np.asarray(a, np.int32), lambda a: np.asarray(a, np.float32)
    dev = Device(gpu, 4, i32(a_rp), i32(a_ci), f32(a_va))
    F = gpu.csr_from_arrays(4, 4, rp, ci, f32(va))                                # a pattern of its own
    assert gpu.csr_to_gpu(F) == 0
    try:
        B = np.ones((4, 3), np.float32)
        X0 = np.arange(12, dtype=np.float32).reshape(4, 3) + 0.5
        results, X = dev.multi(B, X0, ldx=4, F=F)
        assert [r.error_code for r in results] == [gpu.SpMVError.INVALID_ARGUMENT] * 3, case
        assert all((r.iterations, r.converged, r.breakdown) == (0, 0, 0) for r in results)
        assert np.array_equal(bits(X), bits(X0)), case
        ref, _ = dev.single(B[:, 0], X0[:, 0], F=F)
        assert ref.error_code == gpu.SpMVError.INVALID_ARGUMENT                   # cg_solve_ic's own verdict
        results, X = dev.multi(B, X0, ldx=4, F=dev.A)                             # A as its own factor is sound
        assert all(r.error_code == 0 for r in results) and not np.array_equal(bits(X), bits(X0))
    finally:
        gpu.csr_destroy(F)
        dev.close()


def test_a_factor_of_another_size_a_malformed_one_and_the_tiled_engine(gpu):
    E = gpu.SpMVError
    n, rp, ci, va = spd.poisson2d(16)
    dev = Device(gpu, n, rp, ci, va)
    other = Device(gpu, *spd.poisson3d(8))
    bad_ci = ci.copy()
    bad_ci[5] = n + 3
    M = gpu.csr_from_arrays(n, n, rp, bad_ci, va)
    assert gpu.csr_to_gpu(M) == 0
    try:
        B = np.ones((n, 3), np.float32)
        X0 = np.full((n, 3), 0.25, np.float32)
        for kw, code in ((dict(F=other.F), E.INVALID_DIMENSION), (dict(F=M), E.INVALID_FORMAT),
                         (dict(engine=1), E.INVALID_ARGUMENT)):
            results, X = dev.multi(B, X0, ldx=5, **kw)
            assert [r.error_code for r in results] == [code] * 3, kw
            assert all((r.iterations, r.converged, r.breakdown) == (0, 0, 0) for r in results)
            assert np.array_equal(bits(X), bits(X0)), kw
        results, _ = dev.multi(B, X0, engine=-1, preconditioner=7, tolerance=TOL)   # -1 runs the direct kernels;
        assert all(r.error_code == 0 and r.converged for r in results)               # the preconditioner is not read
    finally:
        gpu.csr_destroy(M)
        other.close()
        dev.close()


# ------------------------------------------------------------------------------------------ 9. isolation
def test_the_call_leaves_promotion_and_the_tiled_plan_alone(gpu):
    """test_gpu_cg_multi.test_the_call_leaves_promotion_and_the_tiled_plan_alone for the IC loop: on a tiled-eligible
    matrix neither engine value builds a plan, and VECTOR_CSR calls promote afterwards exactly as on a fresh matrix."""
    n, rp, ci, va = spd.poisson3d(64)
    assert gpu.tiled_shape(n, n, ci.size)[0]
    dev = Device(gpu, n, rp, ci, va)
    saved = gpu.get_tiled_promotion()
    try:
        gpu.set_tiled_promotion(2)
        B = np.random.default_rng(5).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        for engine in (0, -1, 0):
            results, _ = dev.multi(B, np.zeros_like(B), engine=engine, tolerance=1e-6, max_iterations=3)
            assert all((r.error_code, r.iterations) == (0, 3) for r in results)
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
