"""eigs_sym (csrc/eigs.hip) held to the bit on exact data.

tests/test_gpu_eigs.py compares eigs_sym with fp64 eigenvalues and the numpy restatement by measured bounds, which fits
random data and cannot see one unrotated element, one masked tail read wrong or one dropped partial.  Here the data are
built so that the restatement's bits ARE the device's; tests/test_exact_data.py proves every claim about the data
without a GPU (six summation orders of the restatement, the prediction from the walk's tridiagonal matrix alone, the
int64 derivation of the first step, and that every case reaches the grid, lane and basis edge it names).

Tier 1, one-hot Lanczos systems (exact_data.LANCZOS_CASES), tolerance 0, a run that finishes at its FIRST close: every
Lanczos vector is +-e_(q_j), so T, the Ritz pairs and the rotated vectors do not depend on the order of any reduction.
    values, vectors: 0 ulp (NaN values and all-zero rows from `found` on); iterations, restarts, converged, breakdown,
    error_code: equal; the sentinel check of Problem.run at (ldv, offset) = (n, 0) and (n + 3, 1).
    residuals: Problem.check_honest (the project's model bound: a row of A y_i sums three rounded products in a lane-
    dependent order) and max_residual == residuals.max().
    eigs.h admits k < m only, so k >= c runs at m = k + 1 with max_iterations = c (exact_data.lanczos_runs).
Tier 2, the first Lanczos step of every lane count's integer system from a +-1 / 0 start vector
(exact_data.lanczos_first_step): values, vectors, residuals and max_residual 0 ulp, given a correctly rounded fp64
square root on the device (tests/test_gpu_gmres_exact.py assumes the same); counters equal.  The same step at sizes
where the row loop of eigs_spmv<L> takes a second trip (L = 2, 8, 64), and through the tiled engine (0 ulp against the
direct engine and the prediction).
Tier 3, thick restarts of the one-hot systems (exact_data.LANCZOS_RESTART_CASES): after a restart the bits depend on
the order of the dot products (measured on the CPU), so no bit claim but one: every element off the walk is == 0.
    iterations, restarts, found: equal to the restatement's; values within eigs_cases.VALUE_BOUND of the restatement's,
    relative to max |lambda| of the walk's tridiagonal matrix; order, orthonormality within eigs_cases.ortho_bound(k, m)
    and honest residuals as test_gpu_eigs.check_pairs demands them (its `converged == k` cannot hold at tolerance 0:
    converged is held equal to the restatement's 0 instead)."""
import importlib

import numpy as np
import pytest

import eigs_cases as ec
import exact_data as ed

pytestmark = pytest.mark.gpu

eigs_tests = importlib.import_module("test_gpu_eigs")
Problem, bits = eigs_tests.Problem, eigs_tests.bits
LARGEST, SMALLEST = ec.LARGEST, ec.SMALLEST
LAYOUTS = ((0, 0), (3, 1))                     # (ldv - n, offset)
ZERO = np.uint32(0)


def assert_vector_bits(vectors, want, walk, what):
    bad = np.argwhere(bits(vectors) != bits(want))
    at = {int(q): j for j, q in enumerate(walk)} if walk is not None else {}
    assert bad.size == 0, (what, len(bad), [(int(i), int(e), at.get(int(e)), float(vectors[i, e]), float(want[i, e]))
                                            for i, e in bad[:8]])


def assert_pairs_bits(res, values, vectors, residuals, want, walk, what):
    """values and vectors on the bits, NaN / zero rows from `found` on, the counters"""
    found = want["found"]
    assert res.error_code == 0, what
    assert (res.iterations, res.restarts, res.converged, res.breakdown) == \
        (want["iterations"], want["restarts"], want["converged"], want["breakdown"]), \
        (what, res.iterations, res.restarts, res.converged, res.breakdown)
    assert np.array_equal(bits(values[:found]), bits(want["values"][:found])), (what, values, want["values"])
    assert np.all(np.isnan(values[found:])) and np.all(np.isnan(residuals[found:])), what
    assert not np.any(np.isnan(residuals[:found])), what
    assert_vector_bits(vectors, want["vectors"], walk, what)
    assert np.all(bits(vectors[found:]) == ZERO), what


# ------------------------------------------------------------------------------------ 1. one-hot systems, first close
@pytest.mark.parametrize("name", [nm for nm in ed.LANCZOS_NAMES if ed.LANCZOS_CASES[nm]["nan_step"] is None])
def test_onehot_lanczos_run_to_its_first_close_bit_for_bit(gpu, name):
    """eigs_spmv<1>, the three basis kernels, eigs_column, eigs_normalize, eigs_ritz, eigs_rotate<true>, the finish and
    eigs_verdict along the walk of each case, at every (k, m, max_iterations) of the case, both ends of the spectrum and
    two output layouts, against eigs_cases.restate on the walk positions (exact_data.lanczos_onehot_reference)."""
    case, s = ed.lanczos_case(name)
    n = s["n"]
    p = Problem(gpu, n, s["rp"], s["ci"], s["va"])
    try:
        for k, m, cap in case["runs"]:
            for which in (LARGEST, SMALLEST):
                want = ed.lanczos_onehot_reference(s, k, which, m, cap)
                found = want["found"]
                for pad, offset in LAYOUTS:
                    what = (name, k, m, cap, which, pad, offset)
                    res, values, vectors, residuals = p.run(k, which, m, ldv=n + pad, offset=offset, v0=s["v0"],
                                                            tolerance=0.0, max_iterations=cap, engine=0)
                    assert_pairs_bits(res, values, vectors, residuals, want, s["walk"], what)
                    assert res.max_residual == residuals[:found].max(), what
                    if offset == 0:
                        p.check_honest(values[:found], vectors[:found], residuals[:found])
                if case["cut"] is not None:                       # the close the host learns of one step late
                    assert res.iterations == case["cut"] + 1
                    assert res.breakdown == (gpu.EigsResult.INVARIANT_SUBSPACE if k > case["cut"] + 1 else 0)
                else:
                    assert (res.iterations, res.restarts, res.converged, res.breakdown) == (cap, 0, 0, 0)
        assert not gpu.csr_has_tiled_plan(p.A)
    finally:
        p.close()


def test_nan_on_the_walk_fills_every_output_past_the_second_trip(gpu):
    """eigs_fill_failed on 525 315 rows: NOT_FINITE, every value and residual NaN, every vector element +0, the elements
    from 524 288 on included; the guards of both layouts untouched."""
    case, s = ed.lanczos_case("nan_on_the_walk")
    n = s["n"]
    p = Problem(gpu, n, s["rp"], s["ci"], ed.lanczos_nan_values(case, s))
    try:
        (k, m, cap), = case["runs"]
        for pad, offset in LAYOUTS:
            res, values, vectors, residuals = p.run(k, LARGEST, m, ldv=n + pad, offset=offset, v0=s["v0"], tolerance=0.0,
                                                    max_iterations=cap, engine=0)
            assert (res.error_code, res.breakdown, res.converged, res.iterations) == (0, gpu.EigsResult.NOT_FINITE, 0, 0)
            assert np.isnan(res.max_residual)
            assert np.all(np.isnan(values)) and np.all(np.isnan(residuals))
            assert np.all(bits(vectors) == ZERO) and vectors.shape == (k, n) and n > ed.row_trip(1)
    finally:
        p.close()


# ------------------------------------------------------------------------------------ 2. the first step, every lane count
def assert_first_step(gpu, p, v0, step, what, **cfg):
    """one step from a +-1 / 0 start vector: every output against exact_data.lanczos_first_step, 0 ulp"""
    k = ed.LANCZOS_STEP_VALUES
    res, values, vectors, residuals = p.run(k, LARGEST, k + 1, v0=v0, tolerance=0.0, max_iterations=1, **cfg)
    print(what, "value", values[0], step["value"], "residual", residuals[0], step["residual"])
    assert (res.error_code, res.iterations, res.restarts) == (0, 1, 0), what
    assert res.converged == step["converged"], what
    assert res.breakdown == (gpu.EigsResult.INVARIANT_SUBSPACE if step["invariant"] else 0), what
    assert bits(values[0]) == bits(step["value"]), (what, values[0], step["value"])
    assert_vector_bits(vectors[:1], step["vector"][None, :], None, what)
    assert bits(residuals[0]) == bits(step["residual"]), (what, residuals[0], step["residual"])
    assert bits(np.float32(res.max_residual)) == bits(step["residual"]), (what, res.max_residual)
    assert np.all(np.isnan(values[1:])) and np.all(np.isnan(residuals[1:])) and np.all(bits(vectors[1:]) == ZERO), what
    return values, vectors, residuals


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_lanczos_first_step_is_predictable_to_the_bit(gpu, name):
    """eigs_spmv<L, false> and <L, true>, the basis kernels, eigs_residual_partials and eigs_verdict on the integer
    symmetric system of each L: one wrong entry of A v0 moves v0.A v0 or d.d by an integer.  L1_low is the diagonal
    plus one pair with A v0 == v0: INVARIANT_SUBSPACE, value 1, residual 0."""
    L, n, rp, ci, va, v0, step = ed.lanczos_step_system(name)
    p = Problem(gpu, n, rp, ci, va)
    try:
        assert_first_step(gpu, p, v0, step, (name, L), engine=0)
        if name == "L1_low":
            assert (step["value"], step["residual"], step["invariant"]) == (1.0, 0.0, True)
    finally:
        p.close()


@pytest.mark.parametrize("L", ed.LANCZOS_TRIP_LANES)
def test_lanczos_first_step_past_the_row_loops_first_trip(gpu, L):
    """the same step with more rows than 2048 workgroups of 256 / L take: the support of v0 and the non-zeros of A v0
    lie on both sides of row_trip(L) (tests/test_exact_data.py)"""
    n, rp, ci, va, v0, step = ed.lanczos_trip_system(L)
    p = Problem(gpu, n, rp, ci, va)
    try:
        assert_first_step(gpu, p, v0, step, ("trip", L, n), engine=0)
    finally:
        p.close()


def test_lanczos_first_step_through_the_tiled_engine(gpu, monkeypatch):
    """engine 1 at the tiled engine's smallest plan: integer data make every SpMV order exact, so the bits are the
    prediction's and the direct engine's"""
    W, R = ed.ENTRY_POINT_GEOMETRIES[0]
    n, rp, ci, va, v0, step = ed.lanczos_tiled_step_system(W)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    p = Problem(gpu, n, rp, ci, va)
    try:
        direct = assert_first_step(gpu, p, v0, step, ("direct", W, R), engine=0)
        assert not gpu.csr_has_tiled_plan(p.A)
        tiled = assert_first_step(gpu, p, v0, step, ("tiled", W, R), engine=1)
        assert gpu.csr_has_tiled_plan(p.A)
        for a, b in zip(direct, tiled):
            assert np.array_equal(bits(a), bits(b))
    finally:
        p.close()


# ------------------------------------------------------------------------------------ 3. thick restarts
@pytest.mark.parametrize("geometry,k,m", ed.LANCZOS_RESTART_CASES)
def test_thick_restarts_stay_on_the_walk_and_inside_the_bounds(gpu, geometry, k, m):
    """eigs_rotate<false>, eigs_restart and the columns after a restart on elements past 262 144 and 524 288.  The one
    exact claim: nothing can reach an element off the walk, so it is == 0.  The rest by eigs_cases' bounds; the six
    restatement orders lie within VALUE_BOUND / 2 of each other (tests/test_exact_data.py)."""
    s, cap = ed.lanczos_restart_case(geometry, k, m)
    n = s["n"]
    lmax = ed.lanczos_lambda_max(s)
    off_walk = np.ones(n, bool)
    off_walk[s["walk"]] = False
    p = Problem(gpu, n, s["rp"], s["ci"], s["va"])
    try:
        for which in (LARGEST, SMALLEST):
            want = ed.lanczos_onehot_reference(s, k, which, m, cap)
            res, values, vectors, residuals = p.run(k, which, m, v0=s["v0"], tolerance=0.0, max_iterations=cap, engine=0)
            error = float(np.max(np.abs(values.astype(np.float64) - want["values"]))) / lmax
            Y = vectors[:, s["walk"]].astype(np.float64)
            ortho = float(np.max(np.abs(Y @ Y.T - np.eye(k))))
            print(geometry, k, m, which, "steps", res.iterations, "restarts", res.restarts,
                  "value %.2e x lambda_max, ortho %.2e" % (error, ortho))
            assert (res.error_code, res.breakdown) == (0, 0)
            assert (res.iterations, res.restarts) == (want["iterations"], want["restarts"]) and res.restarts >= 1
            assert int(np.count_nonzero(~np.isnan(values))) == want["found"] == k
            assert np.all(bits(vectors[:, off_walk]) == ZERO)
            assert error <= ec.VALUE_BOUND
            # check_pairs but for `converged == k`, which tolerance 0 cannot give
            assert res.converged == want["converged"] == 0
            v64 = values.astype(np.float64)
            assert np.all(np.diff(v64) <= 0) if which == LARGEST else np.all(np.diff(v64) >= 0)
            assert ortho <= ec.ortho_bound(k, m)
            p.check_honest(values, vectors, residuals)
            assert res.max_residual == residuals.max()
    finally:
        p.close()
