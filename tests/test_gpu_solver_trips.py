"""cg_solve, cg_solve_ic, bicgstab_solve, bicgstab_solve_lu and sptrsv_csr past the grid caps, every step to the bit;
and one level schedule through both launch shapes of the level walk (the last section).

csrc/solver_common.h caps the element-wise kernels of the Krylov solvers at 1024 workgroups (V = 262 144 elements a
trip) and the row kernels, sptrsv_kernel on a wide level among them, at 2048 workgroups (R_L = 524 288 / L rows a
trip).  The systems here (tests/exact_data.py, "two-eigenvalue systems" and "two wide levels") are just larger than
that, so every grid-stride loop goes round a second or third time, and they are built so that every quantity of the
documented algorithms is a dyadic rational fp32 holds: x, iterations, converged, breakdown and relative_residual are
known to the bit after one step and after the second, last one, whatever the lane count, grid or fold order.
tests/test_exact_data.py proves that on the CPU by running cg.h's and bicgstab.h's algorithms in integers.

Every comparison is at zero tolerance but one: relative_residual after ONE step is float32(sqrt(r.r) / sqrt(b.b)) of
exact fp64 sums, two square roots and a division the device may round differently from numpy in the last place, so it
may differ from the prediction by one float32 ulp (the rule of tests/test_gpu_gmres_exact.py)."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import precond_trip_cases as pt

pytestmark = pytest.mark.gpu

cg_tests = importlib.import_module("test_gpu_cg")
bicg_tests = importlib.import_module("test_gpu_bicgstab")
sptrsv_tests = importlib.import_module("test_gpu_sptrsv")
multi_tests = importlib.import_module("test_gpu_sptrsv_multi")
ic0_tests = importlib.import_module("test_gpu_ic0")
assert_bits = importlib.import_module("test_gpu_lane_sweep").assert_bits

NONE, JACOBI = 0, 1
TOL = 1e-6
STEPS = 2                                        # both methods end at their second step on two eigenvectors

TRIP_CASES = [(n, 1) for n in ed.TRIP_SIZES]
LANE_CASES = [(ed.LANE_SIZES[L], L) for L in ed.LANES[1:]]
ids = lambda cases: ["n%d_L%d" % c for c in cases]


class Solver:
    """One two-eigenvalue system on the device (test_gpu_bicgstab.System: it runs any of the solvers), with the factor
    matrix of the IC / LU variants next to it."""

    def __init__(self, gpu, system):
        self.gpu, self.system = gpu, system
        self.s = bicg_tests.System(gpu, system["n"], system["rp"], system["ci"], system["va"], b=system["b"])
        self.F = None

    def factor(self, values):
        n = self.system["n"]
        self.F = self.gpu.csr_from_arrays(n, n, *ed.diagonal_csr(values))
        assert self.gpu.csr_to_gpu(self.F) == 0

    def run(self, variant, x0=None, **cfg):
        gpu, s, symmetric = self.gpu, self.s, self.system["symmetric"]
        config = (gpu.CGConfig if symmetric else gpu.BiCGStabConfig)(
            preconditioner=JACOBI if variant == "jacobi" else NONE, **cfg)
        if variant in ("ic", "lu"):
            entry = gpu.cg_solve_ic if symmetric else gpu.bicgstab_solve_lu
            return s._run(lambda A, d_b, d_x, c: entry(A, self.F, d_b, d_x, c), config, x0)
        return s._run(gpu.cg_solve if symmetric else gpu.bicgstab_solve, config, x0)

    def close(self):
        if self.F is not None:
            self.gpu.csr_destroy(self.F)
        self.s.close()


def open_system(gpu, solver, n, L, variant):
    system = ed.two_eig_system(solver, n, L, scaled=variant != "none")
    dev = Solver(gpu, system)
    if variant == "ic":
        dev.factor(np.sqrt(system["diag"]))
    elif variant == "lu":
        dev.factor(system["diag"])
    return system, dev


def assert_two_steps(dev, system, variant, what, engine=0):
    """The full solve and the solve stopped after one step (module docstring)."""
    res, x = dev.run(variant, tolerance=TOL, max_iterations=50, engine=engine)
    what = what + (variant, engine, res.iterations, res.relative_residual)
    assert res.error_code == 0, dev.gpu.spmv_error_string(res.error_code)
    assert res.iterations == STEPS and res.converged == 1 and res.breakdown == 0, what
    assert res.relative_residual == 0.0, what
    assert_bits(system["rp"], x, system["x2"], what)
    res, x = dev.run(variant, tolerance=0.0, max_iterations=1, engine=engine)
    got, want = np.float32(res.relative_residual), system["rel1"]
    ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
    print("one step", what, "relative_residual", got, "predicted", want, "ulps", ulps)
    assert res.error_code == 0 and res.iterations == 1 and res.converged == 0 and res.breakdown == 0, what
    assert_bits(system["rp"], x, system["x1"], what)
    assert ulps <= 1, (what, got, want)


# ------------------------------------------------------------------------------------------ trips and lane counts
@pytest.mark.parametrize("variant", ["none", "jacobi", "ic"])
@pytest.mark.parametrize("n,L", TRIP_CASES, ids=ids(TRIP_CASES))
def test_cg_every_trip(gpu, n, L, variant):
    """cg_init_kernel<1>, cg_spmv_dot<1>, cg_update_kernel<false>, cg_direction_kernel<false> and diag_kernel<POSITIVE>
    below, at and past V, 2 V and R_1; with "ic" the same bits through cg_update_kernel<true>, cg_rz_kernel,
    cg_direction_kernel<true>, diag_kernel<POSITIVE_FINITE> and sptrsv_kernel on the one wide level of the diagonal
    factor.
    From n = 2 V + 3 on both grids sit at their caps and the solve's partial-sum array is 10 240 doubles, a whole number
    of pages: cg_start_kernel once read the double past its end there (the unused neighbour of the last b.b partial),
    which faulted when the next page was not mapped."""
    system, dev = open_system(gpu, "cg", n, L, variant)
    try:
        assert_two_steps(dev, system, variant, ("cg", n, L))
    finally:
        dev.close()


@pytest.mark.parametrize("variant", ["none", "jacobi", "lu"])
@pytest.mark.parametrize("n,L", TRIP_CASES, ids=ids(TRIP_CASES))
def test_bicgstab_every_trip(gpu, n, L, variant):
    """bicg_init_kernel<1>, both bicg_spmv_dot<1> calls, bicg_s_kernel, bicg_update_kernel, bicg_direction_kernel and
    diag_kernel<NONZERO_FINITE> at the same sizes; "lu" is L = I, U = diag(A): JACOBI's bits through the stored p^ / s^."""
    system, dev = open_system(gpu, "bicgstab", n, L, variant)
    try:
        assert_two_steps(dev, system, variant, ("bicgstab", n, L))
    finally:
        dev.close()


@pytest.mark.parametrize("variant", ["none", "jacobi"])
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
@pytest.mark.parametrize("n,L", LANE_CASES, ids=ids(LANE_CASES))
def test_second_row_trip_per_lane_count(gpu, n, L, solver, variant):
    """n = R_L + 256 / L + 1: the row kernels <L> start a second trip with one full workgroup and one of a single row."""
    system, dev = open_system(gpu, solver, n, L, variant)
    try:
        assert_two_steps(dev, system, variant, (solver, n, L))
    finally:
        dev.close()


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
@pytest.mark.parametrize("n,L", LANE_CASES, ids=ids(LANE_CASES))
def test_init_kernel_second_trip_is_exact(gpu, n, L, solver):
    """test_gpu_lane_sweep.test_solver_init_kernel_is_exact at the lane-sweep sizes: b = A x* (exact), x0 = x*, so
    r0 == 0 in every row of both trips of cg_init_kernel<L> / bicg_init_kernel<L>: no step, residual 0.0, x untouched."""
    system = ed.two_eig_system(solver, n, L, scaled=False)
    x_star, b = ed.init_solution(system)
    dev = Solver(gpu, dict(system, b=b))
    try:
        for variant in ("none", "jacobi"):
            res, x = dev.run(variant, x0=x_star, tolerance=1e-5, engine=0)
            what = (solver, n, L, variant, res.iterations, res.relative_residual)
            assert res.error_code == 0 and res.converged and not res.breakdown, what
            assert res.iterations == 0 and res.relative_residual == 0.0, what
            assert_bits(system["rp"], x, x_star, what)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ tiled engine
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_dot_kernels_second_trip_on_the_tiled_engine(gpu, monkeypatch, solver):
    """engine = 1 at n = V + 257: q / v / t come from tiled_spmv and cg_dot_kernel / bicg_dot_kernel (with and without
    the y.y partials) take their second trip.  The same predicted bits as on the direct engine, which runs first."""
    monkeypatch.setenv("SPMV_DEBUG", cg_tests.TILED_SMALL)           # lets the tiled engine take a small matrix
    n = ed.TILED_TRIP_SIZE
    system, dev = open_system(gpu, solver, n, 1, "none")
    try:
        assert_two_steps(dev, system, "none", (solver, n, 1), engine=0)
        assert not gpu.csr_has_tiled_plan(dev.s.A)
        assert_two_steps(dev, system, "none", (solver, n, 1), engine=1)
        assert gpu.csr_has_tiled_plan(dev.s.A)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ sptrsv on its own
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("uplo", [0, 1])
@pytest.mark.parametrize("L", ed.SPTRSV_TRIP_LANES)
def test_sptrsv_two_wide_levels_past_the_grid_cap(gpu, monkeypatch, L, uplo, unit):
    """Two levels of R_L + 256 / L + 1 rows each: sptrsv_kernel<L, false> takes a second trip on both, and at L = 1
    sptrsv_kernel<1, true> (ordered) as well.  x == x* bit for bit, out of place and in place (b and x one array, as
    in the solvers' second triangular solve: there a row that is solved twice no longer gives the same value)."""
    case = ed.two_level_triangle(L, uplo, unit)
    A = sptrsv_tests._upload(gpu, case["n"], case["rp"], case["ci"], case["va"])
    try:
        for ordered in ((0, 1) if L == 1 else (0,)):
            monkeypatch.setenv("SPMV_DEBUG", "sptrsv_lanes=%d" % L)
            cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit, ordered=ordered)
            for in_place in (False, True):
                res, got = sptrsv_tests._solve(gpu, A, case["b"], cfg, in_place=in_place, sentinel=np.nan)
                what = (L, uplo, unit, ordered, in_place, res.num_levels, res.launches, res.lanes_per_row)
                assert res.error_code == 0 and res.num_levels == 2 and res.launches == 2, what
                assert res.lanes_per_row == L, what
                assert_bits(case["rp"], got, case["x"], what)
    finally:
        gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------------ both launch shapes
MIXED_CHAINS = 5                                 # rows of every narrow level
MIXED_K = 5


def narrow_wide_narrow(L, seed=23):
    """(n, rp, ci, va, wide): a symmetric, diagonally dominant forest whose LOWER levels are, in this order, a run of 3
    narrow levels (MIXED_CHAINS rows each), one wide level of kMaxResidentBlocks * (256 / L) + 1 rows and a run of 2
    narrow levels: 3 launches, the first and the last one workgroup each, the wide level's grid at its cap with a
    second trip in which exactly one group is live (its last row, on which a row of the fifth level hangs).
    Every row stores one entry left of the diagonal at most, so IC(0) has no fill to drop and a row's sum is a single
    product: the unordered solves round as the ordered one does, whatever the lane count."""
    m = MIXED_CHAINS
    wide = pt.ROW_BLOCKS * (pt.BLOCK // L) + 1
    head = 3 * m
    n = head + wide + 2 * m
    child = np.arange(m, n, dtype=np.int64)
    parent = child - m                                                  # the chains of levels 0-2, and level 5 on 4
    leaves = np.arange(wide)
    parent[head - m:head - m + wide] = 2 * m + leaves % m               # the wide level hangs on level 2
    parent[head - m + wide:head + wide] = head + np.linspace(0, wide - 1, m).astype(np.int64)   # level 4 on the wide one
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.25, 1.0, child.size) * rng.choice([-1.0, 1.0], child.size)
    idx = np.arange(n, dtype=np.int64)
    diag = 1.0 + np.bincount(child, np.abs(a), n) + np.bincount(parent, np.abs(a), n)
    return pt._assemble(n, [child, parent, idx], [parent, child, idx], [a, a, diag]) + (wide,)


@pytest.mark.parametrize("L", (64, 1))
def test_a_narrow_run_a_wide_level_and_a_narrow_run_in_one_schedule(gpu, monkeypatch, L):
    """One schedule, both launch shapes of for_each_level_row in one solve or factorisation (narrow_wide_narrow):
    sptrsv_csr ordered (and unordered, which runs at the L lanes that give the wide level its second trip),
    sptrsv_csr_multi at k = 5 and ic0_csr at L forced lanes per row, each bit for bit its CPU twin.  8193 wide rows
    at 64 lanes, 524 289 at one lane."""
    n, rp, ci, va, wide = narrow_wide_narrow(L)
    assert wide == {64: 8193, 1: 524289}[L]
    rng = np.random.default_rng(L)
    B = rng.uniform(-1.0, 1.0, (n, MIXED_K)).astype(np.float32)
    dev = multi_tests.Device(gpu, n, rp, ci, va)
    try:
        monkeypatch.setenv("SPMV_DEBUG", "sptrsv_lanes=%d,ic0_lanes=%d" % (L, L))
        shape = lambda res: (res.error_code, res.num_levels, res.launches)
        for ordered in (1, 0):                   # ordered: one lane whatever L; unordered: L lanes, the second trip
            cfg = gpu.SpTRSVConfig(uplo=0, diag=0, ordered=ordered)
            what = ("sptrsv_csr", L, ordered)
            cpu = gpu.sptrsv_cpu_csr(dev.A, B[:, 0], cfg)
            res, x = sptrsv_tests._solve(gpu, dev.A, B[:, 0], cfg, sentinel=np.nan)
            assert shape(res) == (0, 6, 3) and res.lanes_per_row == (1 if ordered else L), what
            assert_bits(rp, x, cpu, what)
        cfg = gpu.SpTRSVConfig(uplo=0, diag=0, ordered=0)
        cpu = np.stack([gpu.sptrsv_cpu_csr(dev.A, B[:, j], cfg) for j in range(MIXED_K)], axis=1)
        res, X = dev.multi(B, cfg)
        what = ("sptrsv_csr_multi", L, res.lanes_per_row)
        assert shape(res) == (0, 6, 3) and res.lanes_per_row == L, what
        np.testing.assert_array_equal(X.view(np.uint32), cpu.view(np.uint32), err_msg=str(what))
        cpu, cpu_pivot = gpu.ic0_cpu_csr(dev.A)
        assert cpu_pivot == -1
        res, got = ic0_tests._factor(gpu, dev.A, va, False)
        what = ("ic0_csr", L, res.lanes_per_row, res.bad_pivot)
        assert shape(res) == (0, 6, 3) and res.lanes_per_row == L and res.bad_pivot == -1, what
        np.testing.assert_array_equal(got.view(np.uint32), cpu.view(np.uint32), err_msg=str(what))
    finally:
        dev.close()
