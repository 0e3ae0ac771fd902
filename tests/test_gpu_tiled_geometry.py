"""The LDS-tiled engine (csrc/tiled.hip) across its plan geometry, on exact data, held to bit equality.

SPMV_DEBUG is read at every use, so each case sets it (monkeypatch.setenv), drops the cached plan and asserts from
csr_tiled_info that the plan really has the strip width, tile height, strip / tile / long-row counts and the folded
or streamed values the case claims (exact_data.GEOMETRY_CASES); tests/test_exact_data.py proves without a GPU that
the data are exact and that the host logic picks that shape.  The data are small integers, the reference is int64,
the comparison is on the bits: NO tolerance anywhere in this file except PageRank's final_residual (4 float32 ulps:
the device sums float32-rounded squares in fp64, takes one square root and rounds once more; see
test_gpu_lane_sweep.test_pagerank_bit_exact_per_lane_count).

spmv_ell builds its plan from the ELL slabs and spmv_csr_transpose's plan belongs to the cached transpose: those two
are read through ell_tiled_info / csr_transpose_tiled_info (a failed build falls back to the direct kernels, which
give the same bits on exact data, so "a plan exists and has this shape" is asserted, not assumed).  The solvers'
tiled route is tested by steps that run tiled_spmv: the first CG, BiCGSTAB and GMRES step, all predictable to
the bit; the r0 == 0 check of the lane sweep is not repeated here, because the init kernels are the direct ones
whatever the engine."""
import importlib

import numpy as np
import pytest

import exact_data as ed

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
cg_tests = importlib.import_module("test_gpu_cg")
bicg_tests = importlib.import_module("test_gpu_bicgstab")
pagerank_tests = importlib.import_module("test_gpu_pagerank")
assert_bits, Device = sweep.assert_bits, sweep.Device
VECTOR, MERGE, ELL = 1, 2, 3
NONE, JACOBI = 0, 1
TILED = 1


def assert_plan(gpu, A, case, info=None):
    """The plan of handle A (or the plan `info` describes) is the one the case claims."""
    items = info["num_items"] if info is not None else (gpu.csr_tiled_items(A) if A is not None else None)
    info = gpu.csr_tiled_info(A) if info is None and A is not None else info
    assert info is not None, "no plan: " + case["name"]
    got = (info["strip_cols"], info["tile_rows"], info["num_strips"], info["num_tiles"], info["values_folded"])
    assert got == (case["W"], case["R"], case["strips"], case["tiles"], case["fold"]), (case["name"], info)
    assert info["long_rows"] == case["long_rows"], (case["name"], info)
    if case.get("slots") is not None:
        assert info["slots_in_cells"] == case["slots"], (case["name"], info)
    if case.get("items") is not None:
        assert items == case["items"], (case["name"], items)
    return info


def run_case(gpu, D, case, rp, x, want, what):
    """VECTOR_CSR and MERGE_PATH with use_texture, twice each: the later calls meet the first one's scratch."""
    for kernel in (VECTOR, MERGE):
        for call in (0, 1):
            assert_bits(rp, D.run(x, kernel, use_texture=True), want, (what, kernel, call))
            assert_plan(gpu, D.A, case)


@pytest.mark.parametrize("name", ed.GEOMETRY_NAMES)
def test_plan_geometry(gpu, monkeypatch, name):
    """Strip width x fold (all eight tiled_expand_kernel instantiations, columns around a strip end), tile heights
    64 .. 9984 (rows around a tile end), every row-delta boundary at R = 9984, phase-1 item boundaries and the
    long-row path at its limit and at the 512-entry chunk boundaries."""
    case, rp, ci, va, x = ed.geometry_matrix(name)
    want = ed.exact_reference(rp, ci, va, x)
    monkeypatch.setenv("SPMV_DEBUG", case["debug"])
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if case["fold"] else "0")
    D = Device(gpu, rp, ci, va, case["cols"])
    try:
        gpu.csr_invalidate_gpu_cache(D.A)
        run_case(gpu, D, case, rp, x, want, name)
        if name.startswith("long_rows"):
            assert gpu.csr_tiled_info(D.A)["long_row_limit"] == ed.LONG_LIMIT
    finally:
        D.close()


@pytest.mark.parametrize("name", ed.BUILDER_FORM_NAMES)
def test_both_builder_forms_against_the_reference(gpu, monkeypatch, name):
    """place=scattered against the staged placing pass, rank=plain against stable binning: equal plan checksums,
    equal bits, and those bits equal to the int64 reference."""
    case, rp, ci, va, x = ed.geometry_matrix(name)
    want = ed.exact_reference(rp, ci, va, x)
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if case["fold"] else "0")
    D = Device(gpu, rp, ci, va, case["cols"])
    try:
        sums = {}
        for form in ("", "place=scattered", "rank=plain", "place=scattered,rank=plain"):
            monkeypatch.setenv("SPMV_DEBUG", case["debug"] + ("," + form if form else ""))
            gpu.csr_invalidate_gpu_cache(D.A)
            run_case(gpu, D, case, rp, x, want, (name, form))
            sums[form] = gpu.csr_tiled_checksum(D.A)
            assert sums[form] is not None and sums[form] == sums[""], (name, form, sums)
    finally:
        D.close()


# ------------------------------------------------------------------------------------------ other entry points
entry_matrix = ed.entry_matrix


def entry_case(what, W, R, rows, cols):
    """The plan of an entry matrix (rows x cols): no long rows (the ELL source has no long-row path; the CSR rows
    are short), values drawn per entry: a value stream."""
    return dict(name="%s_%dx%d" % (what, W, R), W=W, R=R, strips=-(-cols // W), tiles=-(-rows // R), fold=False,
                long_rows=0)


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_ell_source_builder_on_a_forced_geometry(gpu, oracle, monkeypatch, W, R):
    rows, cols, rp, ci, va = entry_matrix(W, R)
    x = np.random.default_rng(1).integers(-64, 65, size=cols).astype(np.float32)
    ed.check_exact(rp, ci, va, x)
    want = ed.exact_reference(rp, ci, va, x)
    kk, ecols, evals = oracle.ell_from_csr(rp, ci, va)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    assert gpu.tiled_shape(rows, cols, rows * kk) == (True, W, R)
    import ctypes
    E = gpu.ell_create(rows, cols, kk)
    ctypes.memmove(E.contents.col_indices, ecols.ctypes.data, ecols.nbytes)
    ctypes.memmove(E.contents.values, evals.ctypes.data, evals.nbytes)
    assert gpu.ell_to_gpu(E) == 0
    d_x, d_y = gpu.CudaBuffer(cols), gpu.CudaBuffer(rows)
    d_x.copyFromHost(x, cols)
    try:
        cfg = gpu.SpMVConfig(kernel_type=ELL, use_texture=True)
        for call in (0, 1):
            d_y.copyFromHost(np.full(rows, sweep.SENTINEL, np.uint32).view(np.float32), rows)
            assert gpu.spmv_ell(E, d_x, d_y, cfg, cols).error_code == 0
            assert_bits(rp, d_y.copyToHost(rows), want, ("ell", W, R, call))
            assert_plan(gpu, None, entry_case("ell", W, R, rows, cols), gpu.ell_tiled_info(E))
    finally:
        gpu.ell_destroy(E)
        d_x.release()
        d_y.release()


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_transposed_spmv_on_a_forced_geometry(gpu, monkeypatch, W, R):
    """y = A^T x with use_texture: the plan belongs to the cached transpose, whose shape is cols x rows.  A is built
    so that A^T has the entry matrix's shape."""
    t_rows, t_cols, t_rp, t_ci, t_va = entry_matrix(W, R)                     # this is A^T
    transpose = importlib.import_module("test_gpu_transpose")
    rp, ci, va = transpose.np_transpose(t_rows, t_cols, t_rp, t_ci, t_va)     # A: t_cols x t_rows
    x = np.random.default_rng(2).integers(-64, 65, size=t_cols).astype(np.float32)
    ed.check_exact(t_rp, t_ci, t_va, x)
    want = ed.exact_reference(t_rp, t_ci, t_va, x)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    assert gpu.tiled_shape(t_rows, t_cols, int(t_rp[-1])) == (True, W, R)
    assert int(np.diff(t_rp).max()) <= ed.default_long_row(-(-t_cols // W))
    M = transpose.Dev(gpu, t_cols, t_rows, rp, ci, va)
    try:
        for kernel in (VECTOR, MERGE):
            for call in (0, 1):
                bits, _ = transpose._run_t(gpu, M, x, gpu.SpMVConfig(kernel, 256, True))
                assert_bits(t_rp, bits.view(np.float32), want, ("transpose", W, R, kernel, call))
                assert_plan(gpu, None, entry_case("transpose", W, R, t_rows, t_cols), gpu.csr_transpose_tiled_info(M.A))
                assert not gpu.csr_has_tiled_plan(M.A)                      # the plan is the transpose's, not A's
    finally:
        M.close()


def solver_case(W, R):
    n = 20011
    strips, tiles = -(-n // W), -(-n // R)
    return dict(name="solver_%dx%d" % (W, R), W=W, R=R, strips=strips, tiles=tiles, fold=False, long_rows=0)


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_cg_first_tiled_step_on_a_forced_geometry(gpu, monkeypatch, W, R):
    """cg_solve with engine = tiled, one step from x0 = 0 without a preconditioner on the integer SPD system: q = A b
    comes from tiled_spmv on the forced plan; p.q = b.q is an integer below 2^53, alpha its quotient rounded to fp32
    and x1[i] == float32(float64(alpha) * b[i]) (test_gpu_lane_sweep.test_cg_first_step_is_predictable_to_the_bit).
    One wrong entry of q moves p.q by an integer, far more than alpha's resolution."""
    n, rp, ci, va = ed.entry_point_systems(W)[0]
    b = np.random.default_rng(W).integers(1, 65, size=n).astype(np.float32)
    ed.check_exact(rp, ci, va, b)
    case = solver_case(W, R)
    assert int(np.diff(rp).max()) <= ed.default_long_row(case["strips"])
    b64 = b.astype(np.int64)
    q = ed.exact_reference(rp, ci, va, b).astype(np.int64)
    assert 0 < int(b64 @ q) < 2**53
    alpha = np.float32(np.float64(int(b64 @ b64)) / np.float64(int(b64 @ q)))
    want = (np.float64(alpha) * b.astype(np.float64)).astype(np.float32)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    s = sweep.system(cg_tests, gpu, n, rp, ci, va, b)
    try:
        for call in (0, 1):                                  # the second solve finds the plan cached
            res, x = s.solve(tolerance=0.0, preconditioner=NONE, engine=TILED, max_iterations=1)
            assert res.error_code == 0 and res.iterations == 1 and not res.converged and not res.breakdown
            assert_plan(gpu, s.A, case)
            assert_bits(rp, x, want, ("cg first step", W, R, float(alpha), call))
    finally:
        s.close()


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_bicgstab_first_tiled_step_on_a_forced_geometry(gpu, monkeypatch, W, R):
    """bicgstab_solve with engine = tiled, one step from x0 = 0 without a preconditioner: both SpMVs of the step
    (v = A p and t = A s) run through tiled_spmv + bicg_dot_kernel on the forced plan.  The system
    (exact_data.bicgstab_first_step_system) makes alpha exactly 1 / 64, so s and t stay exact and x1 is predictable
    to the bit (exact_data.bicgstab_first_step asserts every step of that argument).  A wrong entry of v moves
    rhat.v by an integer, alpha off 1 / 64 and every x1[i]; a wrong entry of t moves omega.  The direct engine runs
    first and must give the same bits: the prediction does not lean on the engine under test."""
    n, rp, ci, va, b = ed.bicgstab_first_step_system(20011, 90000, seed=W)
    want, omega = ed.bicgstab_first_step(rp, ci, va, b)
    case = solver_case(W, R)
    assert int(np.diff(rp).max()) <= ed.default_long_row(case["strips"])
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    s = sweep.system(bicg_tests, gpu, n, rp, ci, va, b)
    try:
        for engine in (0, TILED, TILED):
            res, x = s.solve(tolerance=0.0, preconditioner=NONE, engine=engine, max_iterations=1)
            what = ("bicgstab first step", W, R, engine, float(omega), res.iterations)
            assert res.error_code == 0 and res.iterations == 1 and not res.converged, what
            assert res.breakdown == bicg_tests.NO_BREAKDOWN, what
            if engine == TILED:
                assert_plan(gpu, s.A, case)
            else:
                assert not gpu.csr_has_tiled_plan(s.A)
            assert_bits(rp, x, want, what)
    finally:
        s.close()


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_gmres_first_tiled_step_on_a_forced_geometry(gpu, monkeypatch, W, R):
    """gmres_solve with engine = tiled on the integer non-symmetric system under b = +-1 on 16 384 rows: w = A v_0
    comes from tiled_spmv on the forced plan and x1 must equal exact_data.gmres_first_step's prediction bit for bit
    (test_gpu_gmres_exact.test_gmres_first_step_is_predictable_to_the_bit); the direct engine runs first and must give
    the same bits.  Then restart 2 for four steps: every close runs tiled_spmv into the u buffer and
    gmres_residual_ew, and the cycle after it is opened from that residual.  Past the first step the data are not
    exact, so the engines must agree in iterations and restarts, and in relative_residual within
    test_gpu_gmres.test_engines_agree's rule: SPREAD = 4e-4 of the residual (four times the spread measured between
    two SpMV summation orders, see that module's docstring) plus the rounding bounds of the two recomputed residuals
    (gmres_cases.residual_rounding_bound)."""
    gmres_tests = importlib.import_module("test_gpu_gmres")
    n, rp, ci, va, b = ed.gmres_tiled_step_system(W)
    want, y0 = ed.gmres_first_step(rp, ci, va, b, ed.GMRES_TILED_STEP_K)
    case = solver_case(W, R)
    assert int(np.diff(rp).max()) <= ed.default_long_row(case["strips"])
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    s = gmres_tests.System(gpu, n, rp, ci, va, b=b)
    try:
        for engine in (0, TILED, TILED):                     # the second tiled solve finds the plan cached
            res, x = s.solve(tolerance=0.0, preconditioner=NONE, engine=engine, max_iterations=1)
            what = ("gmres first step", W, R, engine, float(y0), res.iterations)
            assert (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown) == (0, 1, 0, 0, 0), what
            if engine == TILED:
                assert_plan(gpu, s.A, case)
            else:
                assert not gpu.csr_has_tiled_plan(s.A)
            assert_bits(rp, x, want, what)
            gmres_tests.check_honest(s, res, x)
        out = {}
        for engine in (0, TILED):
            res, x = s.solve(tolerance=0.0, preconditioner=NONE, engine=engine, max_iterations=4, restart=2)
            assert (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown) == (0, 4, 1, 0, 0), \
                (W, R, engine, res.iterations, res.restarts)
            gmres_tests.check_honest(s, res, x)
            out[engine] = (float(res.relative_residual), s.bound(x))
        print("gmres restart 2, four steps", W, R, out)
        assert abs(out[TILED][0] - out[0][0]) <= gmres_tests.SPREAD * out[0][0] + out[TILED][1] + out[0][1], out
    finally:
        s.close()


# ------------------------------------------------------------------------------------------ PageRank, bit for bit
def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def assert_dyadic_pagerank(gpu, A, name, want_plan):
    """pagerank() at damping 0.5 for exact_steps steps against integer arithmetic (exact_data.dyadic_pagerank)."""
    n, rp, ci, va, steps, want, residual = ed.dyadic_case(name)
    r = gpu.pagerank(A, gpu.PageRankConfig(ed.DYADIC_DAMPING, 0.0, steps))
    print(name, "steps", steps, "residual", r.final_residual, residual)
    assert r.iterations == steps and not r.converged, (name, r.iterations, steps)
    assert bool(gpu.csr_has_tiled_plan(A)) == want_plan, name
    assert_bits(rp, r.ranks, want, name)
    assert ulps(r.final_residual, np.float32(residual)) <= 4, (name, r.final_residual, residual)


@pytest.mark.parametrize("name", list(ed.DYADIC_TILED))
def test_pagerank_bit_exact_on_the_tiled_engine(gpu, monkeypatch, name):
    """tiled_pagerank_reduce_kernel (fused damping / dangling / teleport update, dangling mask off the folded column
    weights, long-row seeds of the hubs) at three plan geometries, n = 2^16 and 2^18, with dangling nodes (one exact
    step) and without (several), folded values and the value stream; and the switch from the direct kernel to the
    plan after the first step (pr_plan_after=1: only the first of the two calls switches; the second finds the plan
    cached and runs tiled from step 0).  Two calls per graph: the second finds plan and workspace cached.
    The "sources" cases draw their dangling nodes from the nodes nobody links to and stay exact for two or three
    steps: from step 2 on the dangling term is the mass the reduce kernel itself accumulated (block partials ->
    pr_reduce_commit -> state->dangling_sum), which the one-step cases never reach."""
    n, W, R, _, fold, plan_after, _ = ed.DYADIC_TILED[name]
    _, rp, ci, va, steps, _, _ = ed.dyadic_case(name)
    assert steps > plan_after
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, "pr_plan_after=%d" % plan_after))
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if fold else "0")
    case = dict(name=name, W=W, R=R, strips=-(-n // W), tiles=-(-n // R), fold=fold,
                long_rows=int((np.diff(rp) > ed.default_long_row(-(-n // W))).sum()))
    assert case["long_rows"] >= 2
    A = pagerank_tests.upload(gpu, rp, ci, va, n)
    try:
        for _ in range(2):
            assert_dyadic_pagerank(gpu, A, name, want_plan=True)
            assert_plan(gpu, A, case)
    finally:
        gpu.csr_destroy(A)
