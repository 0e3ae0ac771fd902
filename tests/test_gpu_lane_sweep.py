"""Every lanes-per-row kernel instantiation, on exact data, held to bit equality.

pick_lanes_per_row (csrc/kernels.hip) chooses L = 1, 2, 4, 8, 16, 32 or 64 lanes per row from the average row
length for csr_vector_kernel<L>, csr_vector_ldsx_kernel<L>, csr_multi_split_kernel<K, L>, the fused kernels of
cg_solve and bicgstab_solve and pr_step_kernel<L>.  Each L runs here on two matrices, one at the top of its range
(nnz == 4 L rows) and one just past the previous threshold (nnz == 4 (L/2) rows + 1), built from small integers
(tests/exact_data.py): every summation order gives the same bits, so the comparisons with the int64 reference carry
NO tolerance.  tests/test_exact_data.py proves, without a GPU, that each matrix is exact and lands on its L.

Also exact: the merge-path kernels at their tile cut points (tiles of 1 792 merge items, kMergeTile in
csrc/kernels.hip and kMultiTile in csrc/spmm.hip: if the tile size changes, move the shapes of
exact_data.merge_cut_lens) and both ELL kernels at every width remainder.  The solver sweeps reuse the numpy
restatements of test_gpu_cg.py / test_gpu_bicgstab.py and PageRank the parity check of test_gpu_pagerank.py."""
import importlib

import numpy as np
import pytest

import exact_data as ed

pytestmark = pytest.mark.gpu

cg_tests = importlib.import_module("test_gpu_cg")
bicg_tests = importlib.import_module("test_gpu_bicgstab")
pagerank_tests = importlib.import_module("test_gpu_pagerank")
multi_tests = importlib.import_module("test_gpu_spmv_multi")
run_ell = importlib.import_module("test_gpu_spmv").run_ell

SCALAR, VECTOR, MERGE = 0, 1, 2
NONE, JACOBI = 0, 1
SENTINEL = multi_tests.SENTINEL          # a NaN bit pattern no kernel produces by arithmetic


def assert_bits(rp, got, want, what):
    """Bit equality; on a mismatch prints the first rows as (row, got, want, row length, begin % 4)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        rp = np.asarray(rp, np.int64)
        print(what, "%d of %d rows differ:" % (bad.size, want.size),
              [(int(r), float(got[r]), float(want[r]), int(rp[r + 1] - rp[r]), int(rp[r] % 4)) for r in bad[:8]])
    np.testing.assert_array_equal(got, want, err_msg=str(what))


class Device:
    """A CSR matrix on the device and a y buffer one float longer than the matrix has rows."""

    def __init__(self, gpu, rp, ci, va, num_cols):
        self.gpu, self.rp, self.rows, self.num_cols = gpu, rp, len(rp) - 1, num_cols
        self.A = gpu.csr_from_arrays(self.rows, num_cols, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self.d_x = gpu.CudaBuffer(num_cols + 4)
        self.d_y = gpu.CudaBuffer(self.rows + 1)

    def run(self, x, kernel, use_texture=False, x_offset=0):
        """y of one spmv_csr call into a buffer pre-filled with SENTINEL: every row written, nothing past it."""
        gpu, rows = self.gpu, self.rows
        self.d_x.copyFromHost(np.concatenate([np.zeros(x_offset, np.float32), x]), self.num_cols + x_offset)
        self.d_y.copyFromHost(np.full(rows + 1, SENTINEL, np.uint32).view(np.float32), rows + 1)
        cfg = gpu.SpMVConfig(kernel_type=kernel, use_texture=use_texture)
        res = gpu.spmv_csr(self.A, self.d_x.get() + 4 * x_offset, self.d_y, cfg, self.num_cols)
        assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
        y = self.d_y.copyToHost(rows + 1)
        assert y.view(np.uint32)[rows] == SENTINEL, "wrote past the last row"
        return y[:rows]

    def close(self):
        self.gpu.csr_destroy(self.A)


# ------------------------------------------------------------------------------------------ single vector
@pytest.mark.parametrize("name", ed.SWEEP_NAMES)
def test_single_vector_lane_sweep(gpu, name):
    """csr_vector_kernel<L> at both ends of L's range, and MERGE_PATH / SCALAR_CSR on the same matrices."""
    L, rp, ci, va, x = ed.sweep_matrix(name)
    want = ed.exact_reference(rp, ci, va, x)
    D = Device(gpu, rp, ci, va, ed.SWEEP_COLS)
    try:
        for kernel in (VECTOR, MERGE, SCALAR):
            assert_bits(rp, D.run(x, kernel), want, (name, L, kernel))
    finally:
        D.close()


@pytest.mark.parametrize("name", ed.SWEEP_NAMES)
def test_x_in_lds_lane_sweep(gpu, name):
    """csr_vector_ldsx_kernel<L>: use_texture on a matrix that meets vector_ldsx_grid's conditions and stays below
    the tiled engine's column minimum (no plan is built).  x 16-byte aligned and offset by one float: both copy
    loops; the catalogue holds column counts that are and are not multiples of four."""
    L, num_cols, rp, ci, va, x = ed.ldsx_matrix(name)
    want = ed.exact_reference(rp, ci, va, x)
    D = Device(gpu, rp, ci, va, num_cols)
    try:
        for x_offset in (0, 1):
            assert (D.d_x.get() + 4 * x_offset) % 16 == 4 * x_offset
            assert_bits(rp, D.run(x, VECTOR, use_texture=True, x_offset=x_offset), want, (name, L, num_cols, x_offset))
        assert not gpu.csr_has_tiled_plan(D.A)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ spmv_csr_multi
def check_multi(gpu, M, kernel, k, rng, what):
    """X integer, ldx / ldy in {k, k + 3}: every column's bits against the reference, padding columns untouched."""
    for ldx in (k, k + 3):
        X = ed.exact_x_matrix(rng, M.cols, ldx)
        want = [ed.exact_reference(M.rp, M.ci, M.va, np.ascontiguousarray(X[:, j])) for j in range(k)]
        for ldy in (k, k + 3):
            bits, _ = multi_tests._run(gpu, M, X, k, ldx, ldy, kernel)
            assert np.all(bits[:, k:] == SENTINEL), ("padding columns written", what, k, ldx, ldy)
            for j in range(k):
                assert_bits(M.rp, bits.view(np.float32)[:, j], want[j], (what, k, ldx, ldy, j))


@pytest.mark.parametrize("name", ed.SWEEP_NAMES)
def test_multi_vector_lane_sweep(gpu, name):
    """csr_multi_split_kernel<K, L> for K in 1, 2, 3, 4, 8 (35 instantiations over the sweep) and the rows kernel
    through the VECTOR_CSR enum at k = 5 and 16."""
    L, rp, ci, va, _ = ed.sweep_matrix(name)
    M = multi_tests.Host(gpu, len(rp) - 1, ed.SWEEP_COLS, rp, ci, va)
    rng = np.random.default_rng(L)
    try:
        for k in (1, 2, 3, 4, 8, 5, 16):
            check_multi(gpu, M, VECTOR, k, rng, (name, L))
    finally:
        M.close()


# ------------------------------------------------------------------------------------------ merge-path cut points
@pytest.mark.parametrize("name", ed.MERGE_CUT_NAMES)
def test_merge_path_cut_points(gpu, name):
    """merge_tile_kernel + merge_fixup_kernel and csr_multi_merge_tile_kernel<CW> + its fix-up where tile
    boundaries meet row ends, long rows and runs of empty rows (exact_data.merge_cut_lens); k = 1, 2, 3, 4, 7, 8,
    9, 17 take chunk widths 1, 2, 4, 8 and a ragged last chunk."""
    rp, ci, va, x = ed.merge_cut_matrix(name)
    D = Device(gpu, rp, ci, va, ed.MERGE_CUT_COLS)
    try:
        assert_bits(rp, D.run(x, MERGE), ed.exact_reference(rp, ci, va, x), (name, "single"))
    finally:
        D.close()
    M = multi_tests.Host(gpu, len(rp) - 1, ed.MERGE_CUT_COLS, rp, ci, va)
    rng = np.random.default_rng(len(name))
    try:
        for k in (1, 2, 3, 4, 7, 8, 9, 17):
            check_multi(gpu, M, MERGE, k, rng, name)
    finally:
        M.close()


# ------------------------------------------------------------------------------------------ ELL
def test_ell_every_width_remainder_and_row_remainder(gpu, oracle):
    """ell_kernel_x4 (rows % 4 == 0) and ell_kernel_x1 at widths 1..9: the unrolled-by-four loops and every
    remainder of both, exact data, bit equality."""
    for width, rows, rp, ci, va, x in ed.ell_cases():
        kk, ecols, evals = oracle.ell_from_csr(rp, ci, va)
        assert kk == width
        got, _ = run_ell(gpu, rows, 300, kk, ecols, evals, x)
        assert_bits(rp, got, ed.exact_reference(rp, ci, va, x), ("ell", width, rows))


# ------------------------------------------------------------------------------------------ solvers
def system(tests, gpu, n, rp, ci, va, b):
    s = tests.System(gpu, n, rp, ci, va)
    s.b = np.asarray(b, np.float32)
    s.d_b.copyFromHost(s.b, n)
    return s


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_solver_init_kernel_is_exact(gpu, name, solver):
    """cg_init_kernel<L> / bicg_init_kernel<L>: b = A x* (exact), x0 = x*, so r0 = b - A x0 must be exactly zero:
    no step, converged, residual 0.0, x left alone bit for bit."""
    tests = cg_tests if solver == "cg" else bicg_tests
    L, n, rp, ci, va, x_star, _ = ed.solver_system(name, symmetric=(solver == "cg"))
    s = system(tests, gpu, n, rp, ci, va, ed.exact_reference(rp, ci, va, x_star))
    try:
        for precond in (NONE, JACOBI):
            res, x = s.solve(x0=x_star, tolerance=1e-5, preconditioner=precond, engine=0)
            what = (solver, name, L, precond, res.iterations, res.relative_residual)
            assert res.error_code == 0 and res.converged and not res.breakdown, what
            assert res.iterations == 0 and res.relative_residual == 0.0, what
            assert_bits(rp, x, x_star, what)
    finally:
        s.close()


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_cg_first_step_is_predictable_to_the_bit(gpu, name):
    """cg_spmv_dot<L>: from x0 = 0 with an integer b and no preconditioner, p0 = r0 = b and q = A b; r.z = b.b and
    p.q = b.q are integers below 2^53, exact in fp64 under any fold order.  cg.h: alpha is that quotient rounded to
    fp32 and x = fmaf(alpha, p, x), so after one step x1[i] == float32(float64(alpha) * b[i]) (the fp32 product is
    exact in fp64).  One wrong entry of q moves p.q by an integer, far more than alpha's resolution."""
    L, n, rp, ci, va, _, b = ed.solver_system(name, symmetric=True)
    b64 = b.astype(np.int64)
    q = ed.exact_reference(rp, ci, va, b).astype(np.int64)
    alpha = np.float32(np.float64(int(b64 @ b64)) / np.float64(int(b64 @ q)))
    want = (np.float64(alpha) * b.astype(np.float64)).astype(np.float32)
    s = system(cg_tests, gpu, n, rp, ci, va, b)
    try:
        res, x = s.solve(tolerance=0.0, preconditioner=NONE, engine=0, max_iterations=1)
        what = (name, L, float(alpha), res.iterations)
        assert res.error_code == 0 and res.iterations == 1 and not res.converged and not res.breakdown, what
        assert_bits(rp, x, want, what)
    finally:
        s.close()


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_cg_to_convergence_per_lane_count(gpu, name):
    """The assertions of test_gpu_cg.test_restatement_parity on the integer SPD system of each L: iteration count
    within 2 of the restatement, flags, residual below the tolerance, true residual against the real A."""
    L, n, rp, ci, va, _, b = ed.solver_system(name, symmetric=True)
    tol = 1e-5
    s = system(cg_tests, gpu, n, rp, ci, va, b)
    try:
        for precond in (NONE, JACOBI):
            res, x = s.solve(tolerance=tol, preconditioner=precond, engine=0, max_iterations=5000)
            assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
            x_ref, it_ref, conv_ref, brk_ref, _ = cg_tests.restate(n, rp, ci, va, b, np.zeros(n), tol, 5000, precond)
            what = (name, L, precond, res.iterations, it_ref, res.relative_residual)
            print("cg", what)
            assert abs(res.iterations - it_ref) <= 2, what
            assert bool(res.converged) == conv_ref and conv_ref and not res.breakdown and not brk_ref, what
            assert res.relative_residual <= tol, what
            bound = max(4 * tol, 2 * cg_tests.true_residual(rp, ci, va, b, x_ref))
            assert cg_tests.true_residual(rp, ci, va, b, x) <= bound, what
    finally:
        s.close()


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_bicgstab_to_convergence_per_lane_count(gpu, name):
    """The assertions of test_gpu_bicgstab.test_restatement_parity's converged solves on the integer non-symmetric
    system of each L: bicg_spmv_dot<L> with and without the y.y partials."""
    L, n, rp, ci, va, _, b = ed.solver_system(name, symmetric=False)
    tol = 1e-5
    s = system(bicg_tests, gpu, n, rp, ci, va, b)
    try:
        for precond in (NONE, JACOBI):
            res, x = s.solve(tolerance=tol, preconditioner=precond, engine=0, max_iterations=5000)
            assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
            x_ref, it_ref, conv_ref, brk_ref, _ = bicg_tests.restate(n, rp, ci, va, b, np.zeros(n), tol, 5000, precond)
            what = (name, L, precond, res.iterations, it_ref, res.relative_residual)
            print("bicgstab", what)
            assert abs(res.iterations - it_ref) <= max(3, 0.10 * it_ref), what
            assert bool(res.converged) == conv_ref and conv_ref, what
            assert res.breakdown == brk_ref == bicg_tests.NO_BREAKDOWN, what
            assert res.relative_residual <= tol, what
            bound = max(4 * tol, 2 * bicg_tests.true_residual(rp, ci, va, b, x_ref))
            assert bicg_tests.true_residual(rp, ci, va, b, x) <= bound, what
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ PageRank
@pytest.mark.parametrize("name,L,k", ed.PAGERANK_CASES)
def test_pagerank_lane_sweep(gpu, oracle, name, L, k):
    """pr_step_kernel<L> on a graph with k links per row and three dangling nodes, through
    test_gpu_pagerank.assert_parity as it stands.  PageRank's values are reciprocals of link counts, not integers:
    this sweep keeps that check's 1e-5 relative tolerance on every rank; it is the one test here that is not exact."""
    n = ed.PAGERANK_N
    rp, ci, va = ed.pagerank_graph(gpu, pagerank_tests.graph, k, 40 + k)
    assert ed.lanes_for(int(rp[-1]), n) == L
    A = pagerank_tests.upload(gpu, rp, ci, va, n)
    try:
        r = gpu.pagerank(A, gpu.PageRankConfig(0.85, 1e-6, 100))
        assert not gpu.csr_has_tiled_plan(A)
        pagerank_tests.assert_parity(gpu, oracle, A, rp, ci, va, n, r)
    finally:
        gpu.csr_destroy(A)


@pytest.mark.parametrize("name,L,degrees", ed.DYADIC_DIRECT)
def test_pagerank_bit_exact_per_lane_count(gpu, name, L, degrees):
    """pr_step_kernel<L> held to the BIT: n = 2048, damping 0.5, out-degrees powers of two, eight dangling nodes, two
    hub rows, start 1 / n.  Every quantity of r_new = d * (A r) + d * s / n + (1 - d) / n is then a dyadic rational
    of at most 24 bits for exact_steps steps (exact_data.exact_steps proves it on the CPU), so the ranks must equal
    integer arithmetic whatever the summation order, the iteration count is exact and nothing converges at tolerance
    0.  final_residual: the kernel rounds each (r_new - r_old)^2 to float32 (2^-24 relative), sums in fp64 (n * 2^-53),
    takes one square root (halves the relative error) and rounds to float32 once: under 2 ulps; 4 are allowed."""
    n, rp, ci, va, steps, want, residual = ed.dyadic_case(name)
    assert ed.lanes_for(int(rp[-1]), n) == L and steps >= 1
    A = pagerank_tests.upload(gpu, rp, ci, va, n)
    try:
        for _ in range(2):                                  # the second call finds mask and workspace cached
            r = gpu.pagerank(A, gpu.PageRankConfig(ed.DYADIC_DAMPING, 0.0, steps))
            print(name, "steps", steps, "residual", r.final_residual, residual)
            assert r.iterations == steps and not r.converged, (name, r.iterations, steps)
            assert not gpu.csr_has_tiled_plan(A)
            assert_bits(rp, r.ranks, want, name)
            got, exact = np.float32(r.final_residual), np.float32(residual)
            assert abs(int(got.view(np.int32)) - int(exact.view(np.int32))) <= 4, (name, got, residual)
    finally:
        gpu.csr_destroy(A)


@pytest.mark.parametrize("name,L,degrees", ed.DYADIC_SOURCE_DIRECT)
def test_pagerank_device_dangling_mass_bit_exact(gpu, name, L, degrees):
    """pr_step_kernel<L>, L = 1, 2, 4, at n = 2^16 with 4096 dangling nodes that nobody links to: exact for three steps
    (tests/test_exact_data.py), so the dangling term of steps 2 and 3 is the mass the kernel accumulated on the device
    (mass += fresh -> block partials -> pr_reduce_commit -> state->dangling_sum); step 1 takes it from the host.
    Checked after every step count, not only the last."""
    n, rp, ci, va, steps, _, _ = ed.dyadic_case(name)
    assert ed.lanes_for(int(rp[-1]), n) == L and steps >= 2
    trajectory = ed.dyadic_trajectory(rp, ci, va, n, ed.DYADIC_DAMPING, steps)
    A = pagerank_tests.upload(gpu, rp, ci, va, n)
    try:
        for k in list(range(1, steps + 1)) + [steps]:       # the last call finds mask and workspace cached
            want, residual = trajectory[k - 1]
            r = gpu.pagerank(A, gpu.PageRankConfig(ed.DYADIC_DAMPING, 0.0, k))
            print(name, "L", L, "steps", k, "residual", r.final_residual, residual)
            assert r.iterations == k and not r.converged and not gpu.csr_has_tiled_plan(A)
            assert_bits(rp, r.ranks, want, (name, k))
            got, exact = np.float32(r.final_residual), np.float32(residual)
            assert abs(int(got.view(np.int32)) - int(exact.view(np.int32))) <= 4, (name, k, got, residual)
    finally:
        gpu.csr_destroy(A)
