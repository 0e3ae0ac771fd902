"""Every entry point that takes device arrays, on arrays that are VIEWS into larger allocations, held to the bit.

Nearly every other GPU test hands the library what hipMalloc returned: 256-byte aligned, surrounded by untouched slack.
Callers hand it interior pointers (a slice of a global CSR, a vector inside a gathered buffer, raw addresses through
csr_wrap_device / ell_wrap_device).  Here row_ptrs, col_indices, values and every vector start 0..3 elements past a
16-byte boundary (array_views.View) between guards of poison that is legal to read and impossible to overlook:

  * a kernel path that is only right for a 16-byte-aligned base gives a wrong integer;
  * an over-read before a row's begin or past nnz that is USED meets the column poison num_cols - 1, the value poison
    2^22 or the x poison 2^22: x holds non-zero integers, so the row moves by a non-zero integer, mostly by 2^22 or
    more (tests/test_exact_data.py proves it per matrix);
  * a store outside an output vector, before its first element included, breaks a SENTINEL guard.

The data are the exact catalogue's (exact_data.VIEW_NAMES): the reference is int64 and NOTHING here carries a
tolerance.  Every case ends by destroying its wrapped handles, then reading every guard, then freeing the views
(array_views.Views): a wrapped handle owns nothing.

The first test is the smallest: one launch of csr_vector_kernel<1> with only col_indices off the 16-byte boundary, so
that an objection of the hardware to a misaligned 16-byte load would show there, before anything larger runs."""
import ctypes
import importlib

import numpy as np
import pytest

import array_views as av
import exact_data as ed
import exact_triangles
import ic0_cases as ic_cases

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
geometry = importlib.import_module("test_gpu_tiled_geometry")
transpose_tests = importlib.import_module("test_gpu_transpose")
cg_tests = importlib.import_module("test_gpu_cg")
bicg_tests = importlib.import_module("test_gpu_bicgstab")
lu_tests = importlib.import_module("test_gpu_bicgstab_lu")
ic_tests = importlib.import_module("test_gpu_cg_ic")
gmres_tests = importlib.import_module("test_gpu_gmres")
spd = importlib.import_module("gpu-spmv_amd.spd")
nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
assert_bits = sweep.assert_bits

SCALAR, VECTOR, MERGE, ELL = 0, 1, 2, 3
NONE, JACOBI = 0, 1
DIRECT, TILED = 0, 1
SENTINEL = av.SENTINEL
OFFSETS = ed.VIEW_OFFSETS
OFFSET_IDS = ["rp%d_ci%d_va%d" % t for t in OFFSETS]


def spmv_on_views(gpu, A, vx, vy, kernel, num_cols, use_texture=False):
    """One spmv_csr call from x view vx into y view vy (refilled with SENTINEL first); y's payload as float32."""
    vy.upload(np.full(vy.n, SENTINEL, np.uint32).view(np.float32))
    res = gpu.spmv_csr(A, vx.ptr, vy.ptr, gpu.SpMVConfig(kernel_type=kernel, use_texture=use_texture), num_cols)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    return vy.download()


# ------------------------------------------------------------------------------------------ spmv_csr
def test_smallest_case_first_one_misaligned_array_one_launch(gpu):
    """csr_vector_kernel<1> on sweep:L1_low with col_indices one element past a 16-byte boundary and everything else
    aligned: the first misaligned 16-byte global load of this file."""
    m = ed.view_matrix(ed.VIEW_NAMES[0])
    assert m["L"] == 1
    with av.Views(gpu) as V:
        A, _ = V.csr(m["rows"], m["num_cols"], m["rp"], m["ci"], m["va"], (0, 1, 0))
        vx, vy = V.x(m["x"], 0), V.out(m["rows"], 0)
        got = spmv_on_views(gpu, A, vx, vy, VECTOR, m["num_cols"])
        assert_bits(m["rp"], got, ed.exact_reference(m["rp"], m["ci"], m["va"], m["x"]), "first case")


def test_the_helper_itself_places_payloads_and_notices_one_changed_guard_word(gpu):
    """array_views.View at every offset: the address residue, the payload round trip, and check_guards failing when a
    single word before the payload or after it changes (written here with a plain host-to-device copy)."""
    payload = np.arange(1, 38, dtype=np.float32)
    word = np.array([0x12345678], np.uint32)
    for offset in range(4):
        for where in (-1, payload.size, -av.GUARD, payload.size + av.GUARD - 1):
            v = av.View(gpu, payload, offset, SENTINEL)
            try:
                assert v.ptr % 16 == 4 * offset
                np.testing.assert_array_equal(v.download(), payload)
                v.check_guards()
                target = ctypes.c_void_p(v.ptr + 4 * where)
                assert gpu.lib().spmv_c_memcpy_h2d(target, word.ctypes.data_as(ctypes.c_void_p), 4) == 0
                with pytest.raises(AssertionError, match="guard written"):
                    v.check_guards()
                np.testing.assert_array_equal(v.download(), payload)
            finally:
                v.release()


CSR_NAMES = [n for n in ed.VIEW_NAMES if n.split(":")[0] in ("sweep", "merge")]


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("name", CSR_NAMES)
def test_spmv_csr_on_views(gpu, name, offsets):
    """VECTOR_CSR (csr_vector_kernel<L>), MERGE_PATH and SCALAR_CSR; x at every offset, y at an offset that moves with
    it, guards on both sides of y."""
    m = ed.view_matrix(name)
    want = ed.exact_reference(m["rp"], m["ci"], m["va"], m["x"])
    with av.Views(gpu) as V:
        A, _ = V.csr(m["rows"], m["num_cols"], m["rp"], m["ci"], m["va"], offsets)
        xs = [V.x(m["x"], o) for o in range(4)]
        ys = [V.out(m["rows"], o) for o in range(4)]
        for k, kernel in enumerate((VECTOR, MERGE, SCALAR)):
            for xo in range(4):
                yo = (xo + k + offsets[0]) % 4
                got = spmv_on_views(gpu, A, xs[xo], ys[yo], kernel, m["num_cols"])
                assert_bits(m["rp"], got, want, (name, offsets, kernel, xo, yo))
        assert not gpu.csr_has_tiled_plan(A)


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_x_in_lds_kernel_on_views(gpu, offsets):
    """csr_vector_ldsx_kernel<L> (use_texture below the tiled engine's column minimum): both copy loops of x into LDS,
    and no plan."""
    m = ed.view_matrix("ldsx:L4_top")
    want = ed.exact_reference(m["rp"], m["ci"], m["va"], m["x"])
    with av.Views(gpu) as V:
        A, _ = V.csr(m["rows"], m["num_cols"], m["rp"], m["ci"], m["va"], offsets)
        vy = V.out(m["rows"], offsets[2])
        for xo in range(4):
            got = spmv_on_views(gpu, A, V.x(m["x"], xo), vy, VECTOR, m["num_cols"], use_texture=True)
            assert_bits(m["rp"], got, want, ("ldsx", offsets, xo))
        assert not gpu.csr_has_tiled_plan(A)


# ------------------------------------------------------------------------------------------ spmv_csr_multi
@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("name", ["sweep:L4_top", "merge:row_over_four_tiles"])
def test_spmv_csr_multi_on_views(gpu, name, offsets):
    """csr_multi_split_kernel<K, L> (k = 1, 4, 8), the rows kernel (VECTOR_CSR at k = 5) and the merge kernels, with
    ldx % 4 == 0 and X off the 16-byte boundary: `vec` must come out false because of the ADDRESS (the existing sweep
    breaks it through ldx only).  X's padding columns hold the x poison; Y's must keep SENTINEL."""
    m = ed.view_matrix(name)
    rng = np.random.default_rng(sum(offsets))
    with av.Views(gpu) as V:
        A, _ = V.csr(m["rows"], m["num_cols"], m["rp"], m["ci"], m["va"], offsets)
        for i, k in enumerate((1, 4, 8, 5)):
            ld = -(-k // 4) * 4
            X = np.full((m["num_cols"], ld), ed.VIEW_POISON, np.float32)
            X[:, :k] = ed.nonzero_x(rng, m["num_cols"] * k).reshape(m["num_cols"], k)
            want = [ed.exact_reference(m["rp"], m["ci"], m["va"], np.ascontiguousarray(X[:, j])) for j in range(k)]
            xo, yo = 1 + (i + offsets[1]) % 3, 1 + (i + offsets[2]) % 3
            vX, vY = V.x(X.reshape(-1), xo), V.out(m["rows"] * ld, yo)
            for kernel in (VECTOR, MERGE):
                vY.upload(np.full(vY.n, SENTINEL, np.uint32).view(np.float32))
                res = gpu.spmv_csr_multi(A, vX.ptr, vY.ptr, k, ld, ld, gpu.SpMVConfig(kernel), m["num_cols"])
                assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
                Y = vY.download().reshape(m["rows"], ld)
                assert np.all(Y.view(np.uint32)[:, k:] == SENTINEL), ("padding columns written", name, k, kernel)
                for j in range(k):
                    assert_bits(m["rp"], Y[:, j], want[j], (name, offsets, kernel, k, j, xo, yo))


# ------------------------------------------------------------------------------------------ tiled engine
@pytest.fixture(scope="module")
def tiled_member():
    m = ed.view_matrix("tiled:4096x64")
    m["want"] = ed.exact_reference(m["rp"], m["ci"], m["va"], m["x"])
    return m


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_tiled_plan_built_from_csr_views(gpu, monkeypatch, tiled_member, offsets):
    """The plan built from CSR views (a row_ptrs base off the 16-byte boundary takes max_row_kernel's plain loop) has
    the claimed shape and the checksums of the plan built from a csr_to_gpu copy; y equals the int64 reference; the
    same under rank=plain and place=scattered."""
    m = tiled_member
    W, R, rows, cols = m["W"], m["R"], m["rows"], m["num_cols"]
    case = geometry.entry_case("views", W, R, rows, cols)
    monkeypatch.setenv("SPMV_TILED_FOLD", "0")
    D = sweep.Device(gpu, m["rp"], m["ci"], m["va"], cols)
    try:
        with av.Views(gpu) as V:
            A, _ = V.csr(rows, cols, m["rp"], m["ci"], m["va"], offsets)
            vx, vy = V.x(m["x"], offsets[1]), V.out(rows, offsets[2])
            for form in ("", "rank=plain", "place=scattered"):
                monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, form))
                gpu.csr_invalidate_gpu_cache(D.A)
                assert_bits(m["rp"], D.run(m["x"], VECTOR, use_texture=True), m["want"], ("aligned copy", form))
                reference_sums = gpu.csr_tiled_checksum(D.A)
                assert reference_sums is not None
                gpu.csr_invalidate_gpu_cache(A)
                for kernel in (VECTOR, MERGE):
                    got = spmv_on_views(gpu, A, vx, vy, kernel, cols, use_texture=True)
                    geometry.assert_plan(gpu, A, case)
                    assert_bits(m["rp"], got, m["want"], ("tiled csr views", offsets, form, kernel))
                assert gpu.csr_tiled_checksum(A) == reference_sums, (offsets, form)
    finally:
        D.close()


@pytest.mark.parametrize("offsets", [(0, 0), (1, 2), (2, 3), (3, 1)], ids=lambda t: "ci%d_va%d" % t)
def test_tiled_plan_built_from_ell_slab_views(gpu, oracle, monkeypatch, tiled_member, offsets):
    m = tiled_member
    W, R, rows, cols = m["W"], m["R"], m["rows"], m["num_cols"]
    kk, ecols, evals = oracle.ell_from_csr(m["rp"], m["ci"], m["va"])
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    monkeypatch.setenv("SPMV_TILED_FOLD", "0")
    with av.Views(gpu) as V:
        E, _ = V.ell(rows, cols, kk, ecols, evals, offsets)
        vx, vy = V.x(m["x"], offsets[0]), V.out(rows, offsets[1])
        for call in (0, 1):
            vy.upload(np.full(rows, SENTINEL, np.uint32).view(np.float32))
            res = gpu.spmv_ell(E, vx.ptr, vy.ptr, gpu.SpMVConfig(kernel_type=ELL, use_texture=True), cols)
            assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
            geometry.assert_plan(gpu, None, geometry.entry_case("ell views", W, R, rows, cols), gpu.ell_tiled_info(E))
            assert_bits(m["rp"], vy.download(), m["want"], ("tiled ell views", offsets, call))


# ------------------------------------------------------------------------------------------ spmv_ell
def ell_case(width, mod):
    return next((w, rows, rp, ci, va) for w, rows, rp, ci, va, _ in ed.ell_cases() if (w, rows % 4) == (width, mod))


@pytest.mark.parametrize("offsets", [(0, 0), (1, 2), (2, 3), (3, 1)], ids=lambda t: "ci%d_va%d" % t)
@pytest.mark.parametrize("mod", [0, 1], ids=["x4", "x1"])
def test_spmv_ell_on_slab_views(gpu, oracle, mod, offsets):
    """ell_kernel_x4 (rows % 4 == 0: 16-byte loads per slab and a 16-byte store into y) and ell_kernel_x1 at width 9
    (two unrolled rounds and a remainder), slabs, x and y all views."""
    width, rows, rp, ci, va = ell_case(9, mod)
    assert rows % 4 == mod
    x = ed.nonzero_x(np.random.default_rng(mod), 300)
    ed.check_exact(rp, ci, va, x)
    want = ed.exact_reference(rp, ci, va, x)
    kk, ecols, evals = oracle.ell_from_csr(rp, ci, va)
    assert kk == width
    with av.Views(gpu) as V:
        E, _ = V.ell(rows, 300, kk, ecols, evals, offsets)
        for xo in range(4):
            vx, vy = V.x(x, xo), V.out(rows, (xo + offsets[0] + 1) % 4)
            res = gpu.spmv_ell(E, vx.ptr, vy.ptr, None, 300)
            assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
            assert_bits(rp, vy.download(), want, ("ell", mod, offsets, xo))


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_ell_from_csr_gpu_reads_csr_views(gpu, oracle, offsets):
    """The device conversion from CSR views equals the host conversion slab for slab.  (Its output slabs are the
    library's own allocations: the API has no way to hand it a destination.)"""
    width, rows, rp, ci, va = ell_case(9, 1)
    k, want_cols, want_vals = oracle.ell_from_csr(rp, ci, va)
    with av.Views(gpu) as V:
        A, _ = V.csr(rows, 300, rp, ci, va, offsets)
        E = gpu.ell_create(0, 0, 0)
        try:
            assert gpu.ell_from_csr_gpu(E, A) == 0
            e = E.contents
            assert (e.num_rows, e.num_cols, e.max_nnz_per_row) == (rows, 300, k) and e.owns_device_memory
            assert gpu.ell_from_gpu(E) == 0
            got_cols, got_vals = gpu.ell_host_arrays(E)
            np.testing.assert_array_equal(got_cols, want_cols)
            np.testing.assert_array_equal(got_vals.view(np.uint32), want_vals.view(np.uint32))
        finally:
            gpu.ell_destroy(E)


# ------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("name", ["sweep:L4_top", "merge:row_over_four_tiles"])
def test_transpose_of_views(gpu, name, offsets):
    """csr_transpose_gpu of CSR views against the numpy transpose bit for bit, then y = A^T x from an x view into a y
    view through SCALAR_CSR, VECTOR_CSR and MERGE_PATH."""
    m = ed.view_matrix(name)
    rows, cols = m["rows"], m["num_cols"]
    t_rp, t_ci, t_va = transpose_tests.np_transpose(rows, cols, m["rp"], m["ci"], m["va"])
    x = ed.nonzero_x(np.random.default_rng(len(name)), rows)
    ed.check_exact(t_rp, t_ci, t_va, x)
    want = ed.exact_reference(t_rp, t_ci, t_va, x)
    with av.Views(gpu) as V:
        A, _ = V.csr(rows, cols, m["rp"], m["ci"], m["va"], offsets)
        AT, g_rp, g_ci, g_va = transpose_tests.device_transpose(gpu, A)
        try:
            transpose_tests.assert_same_csr((g_rp, g_ci, g_va), (t_rp, t_ci, t_va), (name, offsets))
        finally:
            gpu.csr_destroy(AT)
        for k, kernel in enumerate((SCALAR, VECTOR, MERGE)):
            vx, vy = V.x(x, (k + offsets[1]) % 4), V.out(cols, (k + offsets[2] + 1) % 4)
            res = gpu.spmv_csr_transpose(A, vx.ptr, vy.ptr, gpu.SpMVConfig(kernel), rows)
            assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
            assert_bits(t_rp, vy.download(), want, ("transpose", name, offsets, kernel))


# ------------------------------------------------------------------------------------------ PageRank shard engine
def run_shard(gpu, A, n, mask, r_ptrs, download, steps, damping):
    """One shard engine (spmv_c_pr_shard_create) over handle A: `steps` calls of pr_step_commit between the two
    vectors at r_ptrs, status read after each.  Returns [(ranks, (iterations, residual, converged, done))]."""
    lib = gpu.lib()
    d_mask = gpu.CudaBuffer(n, "uint8")
    d_mask.copyFromHost(mask.astype(np.uint8), n)
    shard = lib.spmv_c_pr_shard_create(A, 0, n, ctypes.c_void_p(d_mask.get()))
    assert shard
    out = []
    try:
        prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
        assert lib.spmv_c_pr_reset(shard, prd.initial_dangling_mass(int(mask.sum()), n), None) == 0
        for k in range(steps):
            old, new = r_ptrs[k & 1], r_ptrs[(k + 1) & 1]
            assert lib.spmv_c_pr_step_commit(shard, ctypes.c_void_p(old), ctypes.c_void_p(new), damping, 0.0, None) == 0
            status = gpu.PrStatus()
            assert lib.spmv_c_pr_status_get(shard, ctypes.byref(status), None) == 0
            out.append((download((k + 1) & 1), (status.iterations, status.final_residual, status.converged, status.done)))
    finally:
        lib.spmv_c_pr_shard_destroy(shard)
        d_mask.release()
    return out


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("engine", ["direct", "tiled"])
def test_pagerank_shard_engine_on_views(gpu, monkeypatch, engine, offsets):
    """One shard engine over matrix views with r_old and r_new as views: pr_step_kernel<L> (direct) and the tiled step
    with pr_plan_after=0.  Five steps bit-equal to the same engine over aligned copies, and for the steps that are
    exact (exact_data.exact_steps) bit-equal to integer arithmetic: the parity check of
    test_gpu_lane_sweep.test_pagerank_bit_exact_per_lane_count."""
    name = "L4" if engine == "direct" else ed.SHARDED_CASE
    n, rp, ci, va, exact, _, _ = ed.dyadic_case(name)
    assert exact >= 1
    trajectory = ed.dyadic_trajectory(rp, ci, va, n, ed.DYADIC_DAMPING, exact)
    if engine == "tiled":
        _, W, R, _, fold, _, _ = ed.DYADIC_TILED[name]
        monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, "pr_plan_after=0"))
        monkeypatch.setenv("SPMV_TILED_FOLD", "1" if fold else "0")
    mask = np.bincount(ci, minlength=n) == 0
    start = np.full(n, np.float32(1.0) / np.float32(n), np.float32)
    steps = 5
    # aligned copies
    A0 = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A0) == 0
    bufs = [gpu.CudaBuffer(n), gpu.CudaBuffer(n)]
    try:
        for b in bufs:
            b.copyFromHost(start, n)
        plain = run_shard(gpu, A0, n, mask, [b.get() for b in bufs], lambda i: bufs[i].copyToHost(n), steps,
                          ed.DYADIC_DAMPING)
        assert bool(gpu.csr_has_tiled_plan(A0)) == (engine == "tiled")
    finally:
        gpu.csr_destroy(A0)
        for b in bufs:
            b.release()
    with av.Views(gpu) as V:
        A, _ = V.csr(n, n, rp, ci, va, offsets)
        r = [V.view(start, offsets[1], SENTINEL), V.view(start, offsets[2], SENTINEL)]
        got = run_shard(gpu, A, n, mask, [v.ptr for v in r], lambda i: r[i].download(), steps, ed.DYADIC_DAMPING)
        assert bool(gpu.csr_has_tiled_plan(A)) == (engine == "tiled")
        for k in range(steps):
            assert got[k][1] == plain[k][1] and got[k][1][0] == k + 1, (engine, offsets, k, got[k][1], plain[k][1])
            assert_bits(rp, got[k][0], plain[k][0], (engine, offsets, "against aligned copies, step", k + 1))
            if k < exact:
                want, residual = trajectory[k]
                assert_bits(rp, got[k][0], want, (engine, offsets, "against integers, step", k + 1))
                assert geometry.ulps(got[k][1][1], np.float32(residual)) <= 4, (engine, k, got[k][1], residual)


# ------------------------------------------------------------------------------------------ cg_solve, bicgstab_solve
def solve_on_views(gpu, V, solver, config, n, rp, ci, va, b, offsets, b_off, x_off):
    A, _ = V.csr(n, n, rp, ci, va, offsets)
    vb = V.x(b, b_off)
    vx = V.view(np.zeros(n, np.float32), x_off, SENTINEL)
    res = solver(A, vb.ptr, vx.ptr, config)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    return A, res, vx.download()


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("engine", [DIRECT, TILED], ids=["direct", "tiled"])
def test_cg_first_step_on_views(gpu, monkeypatch, engine, offsets):
    """cg_solve at max_iterations = 1 on the integer SPD system of test_gpu_tiled_geometry, predictable to the bit
    (test_gpu_lane_sweep.test_cg_first_step_is_predictable_to_the_bit): the fused direct kernels and tiled_spmv."""
    W, R = ed.ENTRY_POINT_GEOMETRIES[0]
    n, rp, ci, va = ed.entry_point_systems(W)[0]
    b = np.random.default_rng(W).integers(1, 65, size=n).astype(np.float32)
    b64 = b.astype(np.int64)
    q = ed.exact_reference(rp, ci, va, b).astype(np.int64)
    alpha = np.float32(np.float64(int(b64 @ b64)) / np.float64(int(b64 @ q)))
    want = (np.float64(alpha) * b.astype(np.float64)).astype(np.float32)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    with av.Views(gpu) as V:
        cfg = gpu.CGConfig(tolerance=0.0, max_iterations=1, preconditioner=NONE, engine=engine)
        A, res, x = solve_on_views(gpu, V, gpu.cg_solve, cfg, n, rp, ci, va, b, offsets, offsets[1], offsets[2])
        assert res.iterations == 1 and not res.converged and not res.breakdown
        if engine == TILED:
            geometry.assert_plan(gpu, A, geometry.solver_case(W, R))
        else:
            assert not gpu.csr_has_tiled_plan(A)
        assert_bits(rp, x, want, ("cg first step", engine, offsets, float(alpha)))


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("engine", [DIRECT, TILED], ids=["direct", "tiled"])
def test_bicgstab_first_step_on_views(gpu, monkeypatch, engine, offsets):
    """bicgstab_solve at max_iterations = 1 on exact_data.bicgstab_first_step_system: both SpMVs of the step."""
    W, R = ed.ENTRY_POINT_GEOMETRIES[0]
    n, rp, ci, va, b = ed.bicgstab_first_step_system(20011, 90000, seed=W)
    want, omega = ed.bicgstab_first_step(rp, ci, va, b)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    with av.Views(gpu) as V:
        cfg = gpu.BiCGStabConfig(tolerance=0.0, max_iterations=1, preconditioner=NONE, engine=engine)
        A, res, x = solve_on_views(gpu, V, gpu.bicgstab_solve, cfg, n, rp, ci, va, b, offsets, offsets[2], offsets[1])
        assert res.iterations == 1 and not res.converged and res.breakdown == bicg_tests.NO_BREAKDOWN
        if engine == TILED:
            geometry.assert_plan(gpu, A, geometry.solver_case(W, R))
        else:
            assert not gpu.csr_has_tiled_plan(A)
        assert_bits(rp, x, want, ("bicgstab first step", engine, offsets, float(omega)))


@pytest.mark.parametrize("offsets", OFFSETS[1:], ids=OFFSET_IDS[1:])
@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
def test_full_solve_on_views_equals_the_solve_on_aligned_copies(gpu, solver, offsets):
    """poisson2d(64) to convergence with the Jacobi preconditioner: iterations, flags, residual and every bit of x."""
    n, rp, ci, va = spd.poisson2d(64)
    b = np.random.default_rng(9).uniform(-1.0, 1.0, n).astype(np.float32)
    s = bicg_tests.System(gpu, n, rp, ci, va, b=b)
    try:
        run = s.cg if solver == "cg" else s.solve
        ref, x_ref = run(tolerance=1e-6, preconditioner=JACOBI, engine=DIRECT)
    finally:
        s.close()
    assert ref.error_code == 0 and ref.converged and ref.iterations > 10
    with av.Views(gpu) as V:
        if solver == "cg":
            call, cfg = gpu.cg_solve, gpu.CGConfig(tolerance=1e-6, preconditioner=JACOBI, engine=DIRECT)
        else:
            call, cfg = gpu.bicgstab_solve, gpu.BiCGStabConfig(tolerance=1e-6, preconditioner=JACOBI, engine=DIRECT)
        _, res, x = solve_on_views(gpu, V, call, cfg, n, rp, ci, va, b, offsets, offsets[0], offsets[2])
        got = (res.iterations, res.converged, res.breakdown, res.relative_residual)
        assert got == (ref.iterations, ref.converged, ref.breakdown, ref.relative_residual), (solver, offsets)
        assert_bits(rp, x, x_ref, (solver, "full solve", offsets))


# ------------------------------------------------------------------------------------------ sptrsv, ilu0, LU
TRIANGLE_SPECS = {"lower_pow2_diagonal": (1, 0, 0, [700, 40, 300, 5, 5, 5, 900, 257, 256, 10, 1, 1, 600]),
                  "upper_unit_diagonal": (4, 1, 1, [300, 3, 3, 3, 1000, 17, 64, 65, 2])}      # test_gpu_sptrsv.EXACT_SPECS
_triangles = {}


def triangle(name):
    if name not in _triangles:
        _triangles[name] = exact_triangles.cases([TRIANGLE_SPECS[name]])[0]
    return _triangles[name]
LANE_COUNTS = (1, 4, 64)


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
@pytest.mark.parametrize("triangle_name", list(TRIANGLE_SPECS))
def test_sptrsv_on_views(gpu, monkeypatch, triangle_name, offsets):
    """sptrsv_csr ORDERED against sptrsv_cpu_csr, and at 1, 4 and 64 lanes per row on exact integer triangles
    (tests/exact_triangles.py) against the integer solution, out of place and in place, all at zero tolerance."""
    case = triangle(triangle_name)
    assert exact_triangles.prove(case)
    b, want = case.b.astype(np.float32), case.x.astype(np.float32)
    host = gpu.csr_from_arrays(case.n, case.n, case.rp, case.ci, case.va)
    try:
        cpu = gpu.sptrsv_cpu_csr(host, b, gpu.SpTRSVConfig(uplo=case.uplo, diag=case.unit, ordered=1))
    finally:
        gpu.csr_destroy(host)
    np.testing.assert_array_equal(cpu.view(np.uint32), want.view(np.uint32))
    with av.Views(gpu) as V:
        A, _ = V.csr(case.n, case.n, case.rp, case.ci, case.va, offsets)
        for i, (ordered, lanes) in enumerate([(1, 1)] + [(0, L) for L in LANE_COUNTS]):
            monkeypatch.setenv("SPMV_DEBUG", "sptrsv_lanes=%d" % lanes)
            cfg = gpu.SpTRSVConfig(uplo=case.uplo, diag=case.unit, ordered=ordered)
            vb = V.x(b, (i + offsets[1]) % 4)
            vx = V.out(case.n, (i + offsets[2]) % 4)
            res = gpu.sptrsv_csr(A, vb.ptr, vx.ptr, cfg)
            tag = (case.name, offsets, ordered, lanes)
            assert res.error_code == 0 and res.lanes_per_row == lanes and res.num_levels == len(case.widths), tag
            assert_bits(case.rp, vx.download(), want, tag)
            res = gpu.sptrsv_csr(A, vb.ptr, vb.ptr, cfg)                       # in place
            assert res.error_code == 0, tag
            assert_bits(case.rp, vb.download(), want, tag + ("in place",))


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_ilu0_and_lu_preconditioned_bicgstab_on_views(gpu, monkeypatch, offsets):
    """ilu0_csr at 1, 4 and 64 lanes per row into a d_lu view and in place over the values view, against ilu0_cpu_csr
    at zero tolerance; then bicgstab_solve_lu with LU wrapped over the structure views and the d_lu view: iterations
    and x bit-equal to the run on aligned copies."""
    n, rp, ci, va = nonsym.convdiff2d(24, (3.0, 0.5))
    nnz = int(ci.size)
    b = np.random.default_rng(5).uniform(-1.0, 1.0, n).astype(np.float32)
    s = lu_tests.LUSystem(gpu, n, rp, ci, va, b=b)
    try:
        want = s.lu.copy()
        ref, x_ref = s.solve_lu(tolerance=1e-6, engine=DIRECT)
    finally:
        s.close()
    assert ref.error_code == 0 and ref.converged and ref.iterations >= 2
    with av.Views(gpu) as V:
        A, (v_rp, v_ci, v_va) = V.csr(n, n, rp, ci, va, offsets)
        for i, lanes in enumerate(LANE_COUNTS):
            monkeypatch.setenv("SPMV_DEBUG", "ilu0_lanes=%d" % lanes)
            d_lu = V.out(nnz, (i + offsets[0] + 1) % 4)
            res = gpu.ilu0_csr(A, d_lu.ptr)
            tag = ("ilu0", offsets, lanes)
            assert res.error_code == 0 and res.zero_pivot == -1 and res.lanes_per_row == lanes, tag
            np.testing.assert_array_equal(d_lu.download().view(np.uint32), want.view(np.uint32), err_msg=str(tag))
            res = gpu.ilu0_csr(A, v_va.ptr)                                   # in place over the values view
            assert res.error_code == 0 and res.zero_pivot == -1, tag
            np.testing.assert_array_equal(v_va.download().view(np.uint32), want.view(np.uint32), err_msg=str(tag))
            v_va.upload(va)
            gpu.csr_invalidate_gpu_cache(A)
        monkeypatch.delenv("SPMV_DEBUG")
        LU = gpu.csr_wrap_device(n, n, nnz, v_rp.ptr, v_ci.ptr, d_lu.ptr)
        V.csr_handles.append(LU)
        vb, vx = V.x(b, offsets[2]), V.view(np.zeros(n, np.float32), offsets[1], SENTINEL)
        res = gpu.bicgstab_solve_lu(A, LU, vb.ptr, vx.ptr, gpu.BiCGStabConfig(tolerance=1e-6, engine=DIRECT))
        got = (res.error_code, res.iterations, res.converged, res.breakdown, res.relative_residual)
        assert got == (0, ref.iterations, ref.converged, ref.breakdown, ref.relative_residual), (offsets, got)
        assert_bits(rp, vx.download(), x_ref, ("bicgstab_solve_lu", offsets))


# ------------------------------------------------------------------------------------------ ic0, IC-CG, GMRES
@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_ic0_and_ic_preconditioned_cg_on_views(gpu, offsets):
    """ic0_csr of a view-backed A into a view and in place over the values view, against the factor of the aligned copy
    (which test_gpu_cg_ic.ICSystem holds to ic0_cpu_csr) at zero tolerance; then cg_solve_ic with A, the factor, b and
    x all views: iterations, flags, residual and every bit of x as on aligned copies.  1203 rows: 3 mod 4."""
    n, rp, ci, va = ic_cases.sorted_random_spd(1203, 7, seed=21)
    nnz = int(ci.size)
    assert n % 4 == 3
    b = np.random.default_rng(6).uniform(-1.0, 1.0, n).astype(np.float32)
    s = ic_tests.ICSystem(gpu, n, rp, ci, va, b=b)
    try:
        want = s.l.copy()
        ref, x_ref = s.solve_ic(tolerance=1e-6, engine=DIRECT)
    finally:
        s.close()
    assert ref.error_code == 0 and ref.converged and ref.iterations >= 2
    with av.Views(gpu) as V:
        A, (v_rp, v_ci, v_va) = V.csr(n, n, rp, ci, va, offsets)
        d_l = V.out(nnz, (offsets[0] + 1) % 4)
        res = gpu.ic0_csr(A, d_l.ptr)
        assert res.error_code == 0 and res.bad_pivot == -1, offsets
        np.testing.assert_array_equal(d_l.download().view(np.uint32), want.view(np.uint32), err_msg=str(offsets))
        V.check_guards(("ic0_csr", offsets))
        res = gpu.ic0_csr(A, v_va.ptr)                                        # in place over the values view
        assert res.error_code == 0 and res.bad_pivot == -1, offsets
        np.testing.assert_array_equal(v_va.download().view(np.uint32), want.view(np.uint32), err_msg=str(offsets))
        V.check_guards(("ic0_csr in place", offsets))
        v_va.upload(va)
        gpu.csr_invalidate_gpu_cache(A)
        F = gpu.csr_wrap_device(n, n, nnz, v_rp.ptr, v_ci.ptr, d_l.ptr)
        V.csr_handles.append(F)
        vb, vx = V.x(b, offsets[2]), V.view(np.zeros(n, np.float32), offsets[1], SENTINEL)
        res = gpu.cg_solve_ic(A, F, vb.ptr, vx.ptr, gpu.CGConfig(tolerance=1e-6, engine=DIRECT))
        got = (res.error_code, res.iterations, res.converged, res.breakdown, res.relative_residual)
        assert got == (0, ref.iterations, ref.converged, ref.breakdown, ref.relative_residual), (offsets, got)
        assert_bits(rp, vx.download(), x_ref, ("cg_solve_ic", offsets))
        V.check_guards(("cg_solve_ic", offsets))


@pytest.mark.parametrize("offsets", OFFSETS, ids=OFFSET_IDS)
def test_gmres_and_lu_preconditioned_gmres_on_views(gpu, offsets):
    """gmres_solve (NONE, JACOBI) and gmres_solve_lu on the convection-diffusion system (ascending columns, which
    ilu0_csr wants) with A's three arrays, the factor's values, b and x all views: iterations, restarts, flags, the
    bits of relative_residual and every bit of x as on aligned copies.  1089 rows: 1 mod 4; restart 9 restarts."""
    n, rp, ci, va = nonsym.convdiff2d(33, 3.0)
    nnz = int(ci.size)
    same_row = np.diff(np.repeat(np.arange(n), np.diff(rp))) == 0
    assert n % 4 == 1 and np.all(np.diff(ci)[same_row] > 0)
    s = gmres_tests.System(gpu, n, rp, ci, va)
    b = s.b
    try:
        lu = s.factor()
        want_lu = s.d_lu.copyToHost(nnz)
        plain = {}
        for kind in ("none", "jacobi", "lu"):
            plain[kind] = s.solve(LU=lu if kind == "lu" else None, tolerance=1e-6, restart=9, engine=DIRECT,
                                  preconditioner=JACOBI if kind == "jacobi" else NONE)
            assert plain[kind][0].error_code == 0 and plain[kind][0].converged, kind
        assert plain["none"][0].restarts >= 1
    finally:
        s.close()
    with av.Views(gpu) as V:
        A, (v_rp, v_ci, v_va) = V.csr(n, n, rp, ci, va, offsets)
        d_lu = V.out(nnz, (offsets[0] + 2) % 4)
        res = gpu.ilu0_csr(A, d_lu.ptr)
        assert res.error_code == 0 and res.zero_pivot == -1, offsets
        np.testing.assert_array_equal(d_lu.download().view(np.uint32), want_lu.view(np.uint32), err_msg=str(offsets))
        LU = gpu.csr_wrap_device(n, n, nnz, v_rp.ptr, v_ci.ptr, d_lu.ptr)
        V.csr_handles.append(LU)
        for i, kind in enumerate(("none", "jacobi", "lu")):
            cfg = gpu.GMRESConfig(tolerance=1e-6, restart=9, engine=DIRECT,
                                  preconditioner=JACOBI if kind == "jacobi" else NONE)
            vb = V.x(b, (i + offsets[2]) % 4)
            vx = V.view(np.zeros(n, np.float32), (i + offsets[1]) % 4, SENTINEL)
            res = gpu.gmres_solve_lu(A, LU, vb.ptr, vx.ptr, cfg) if kind == "lu" else \
                gpu.gmres_solve(A, vb.ptr, vx.ptr, cfg)
            ref, x_ref = plain[kind]
            got = (res.error_code, res.iterations, res.restarts, res.converged, res.breakdown)
            assert got == (0, ref.iterations, ref.restarts, ref.converged, ref.breakdown), (kind, offsets, got)
            assert np.float32(res.relative_residual).view(np.uint32) == np.float32(ref.relative_residual).view(np.uint32)
            assert_bits(rp, vx.download(), x_ref, ("gmres", kind, offsets))
            V.check_guards(("gmres", kind, offsets))
        assert not gpu.csr_has_tiled_plan(A)
