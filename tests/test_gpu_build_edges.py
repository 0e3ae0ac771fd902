"""The kernels the matrix builders share (csrc/csr_build.hip) at every scan, block and grid edge, through
the public API, at zero tolerance.

The scan: every caller (csr_add, csr_permute_gpu, spgemm_csr, fsai_csr, csr_from_coo_gpu, amg_aggregate_mis2_gpu and
amg_setup_device, csr_transpose_gpu) at lengths on and around one and two tiles of 4096, on row lengths that make a
carry from the wrong tile, a lost carry or a lost total visible (build_edge_cases.edge_profile); csr_add,
csr_permute_gpu and spgemm_csr on and just past 4096^2 elements, where the recursion goes three deep.  row_of[p] with
rows that end on, span and skip the 256 entries of a workgroup.  The structure check with its defect past the 524 288
work items of one trip, in both regimes, through every door.  iota past its grid.

The structure is compared with numpy (cumsum, repeat, unique, a stable argsort), all three arrays with the host twin.
tests/test_build_edge_cases_host.py proves what each case is named for."""
import numpy as np
import pytest

import array_views as av
import build_edge_cases as bc
import fsai_cases as fc
import mis2_cases as mc
import reorder_cases as rc
from test_gpu_amg import Hier, assert_levels_equal
from test_gpu_amg_setup_device import DeviceHier, definition_maps

pytestmark = pytest.mark.gpu

POISON = np.int32(-77)
COLS = 16


def _upload(gpu, rows, cols, arrays):
    M = gpu.csr_from_arrays(rows, cols, *arrays)
    assert gpu.csr_to_gpu(M) == 0
    return M


def _int_buffer(gpu, values):
    values = np.ascontiguousarray(values, np.int32)
    buf = gpu.CudaBuffer(max(values.size, 1), "int32")
    if values.size:
        buf.copyFromHost(values, values.size)
    return buf


def _float_buffer(gpu, values):
    values = np.ascontiguousarray(values, np.float32)
    buf = gpu.CudaBuffer(max(values.size, 1))
    if values.size:
        buf.copyFromHost(values, values.size)
    return buf


def _same(got, want, what):
    for g, w, part in zip(got, want, ("row_ptrs", "col_indices", "values")):
        assert np.asarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, part)


def _device_result(gpu, C, rows, cols):
    m = C.contents
    assert (m.num_rows, m.num_cols) == (rows, cols) and m.owns_device_memory
    assert gpu.csr_from_gpu(C) == 0
    return gpu.csr_host_arrays(C)


# ---- the callers of the scan: name -> (gpu, size) -> None ---------------------------------------------------------
def _add(gpu, rows):
    a, b = bc.add_pair(rows, COLS)
    A, B = _upload(gpu, rows, COLS, a), _upload(gpu, rows, COLS, b)
    C, H = gpu.csr_create(3, 3, 2), gpu.csr_create(0, 0, 0)
    try:
        res = gpu.csr_add(C, 1.5, A, -0.75, B)
        assert res.error_code == 0
        got = _device_result(gpu, C, rows, COLS)
        rp, ci = bc.np_add_structure(rows, COLS, a, b)
        _same(got[:2], (rp, ci), ("csr_add against numpy", rows))
        assert gpu.csr_add_cpu(H, 1.5, A, -0.75, B) == 0
        _same(got, gpu.csr_host_arrays(H), ("csr_add against csr_add_cpu", rows))
        assert res.nnz == ci.size > 0 and got[0][rows] == ci.size
        # the depth that ran: the counting pass, the scan's 1, 3 or 5 kernels, the numeric pass
        depth = bc.scan_depth(rows + 1)
        assert res.launches == 1 + (1, 3, 5)[depth - 1] + 1 == 2 + bc.scan_launches(bc.scan_levels(rows + 1))
    finally:
        for M in (A, B, C, H):
            gpu.csr_destroy(M)


def _permute(gpu, rows):
    a = bc.short_rows_from(bc.edge_profile(rows, seed=4), 14, COLS)
    A = _upload(gpu, rows, COLS, a)
    B, H = gpu.csr_create(3, 3, 2), gpu.csr_create(0, 0, 0)
    reversal = np.arange(rows, dtype=np.int32)[::-1].copy()
    try:
        for perm in ((reversal, None) if rows <= bc.SCAN_ROWS[-1] else (reversal,)):
            d_perm = None if perm is None else _int_buffer(gpu, perm)
            assert gpu.csr_permute_gpu(B, A, d_perm, None) == 0
            if d_perm is not None:
                d_perm.release()
            got = _device_result(gpu, B, rows, COLS)
            want = bc.np_permute_rows(a, np.arange(rows) if perm is None else perm)
            _same(got, want, ("csr_permute_gpu against numpy", rows, perm is None))
            assert gpu.csr_permute_cpu(H, A, perm, None) == 0
            _same(got, gpu.csr_host_arrays(H), ("csr_permute_gpu against csr_permute_cpu", rows, perm is None))
    finally:
        for M in (A, B, H):
            gpu.csr_destroy(M)


def _product(gpu, m):
    k, n = 16, 64
    a, b = bc.product_pair(m, k, n)
    A, B = _upload(gpu, m, k, a), _upload(gpu, k, n, b)
    C, H = gpu.csr_create(3, 3, 2), gpu.csr_create(0, 0, 0)
    try:
        res = gpu.spgemm_csr(C, A, B)
        assert res.error_code == 0
        got = _device_result(gpu, C, m, n)
        rp, ci = bc.np_product_structure(m, n, a, b)
        _same(got[:2], (rp, ci), ("spgemm_csr against numpy", m))
        assert gpu.spgemm_cpu_csr(H, A, B) == 0
        _same(got, gpu.csr_host_arrays(H), ("spgemm_csr against spgemm_cpu_csr", m))
        bound = bc.product_bounds(a, b)
        classes = [int((bound == 0).sum()), int(((bound > 0) & (bound <= 16)).sum()), int((bound > 16).sum())]
        assert list(res.symbolic_rows[:3]) == classes and min(classes) > 0 and sum(classes) == m
        assert res.nnz == ci.size == got[0][m]
    finally:
        for M in (A, B, C, H):
            gpu.csr_destroy(M)


def _fsai(gpu, n):
    _, rp, ci, va = fc.banded_spd(n, 2)
    A = _upload(gpu, n, n, (rp, ci, va))
    G, H = gpu.csr_create(3, 3, 2), gpu.csr_create(0, 0, 0)
    try:
        res = gpu.fsai_csr(G, A)
        assert res.error_code == 0 and res.bad_row == -1
        got = _device_result(gpu, G, n, n)
        g_rp, g_ci = fc.lower_pattern(n, rp, ci)
        _same(got[:2], (g_rp, g_ci), ("fsai_csr against the lower pattern", n))
        assert gpu.fsai_cpu_csr(H, A) == (0, -1)
        _same(got, gpu.csr_host_arrays(H), ("fsai_csr against fsai_cpu_csr", n))
        assert res.nnz == g_ci.size == 3 * n - 3
    finally:
        for M in (A, G, H):
            gpu.csr_destroy(M)


def _from_coo(gpu, count):
    rows, cols = 700, 40
    r, c, v = bc.coo_triplets(count, rows, cols)
    bufs = [_int_buffer(gpu, r), _int_buffer(gpu, c), _float_buffer(gpu, v)]
    C, H = gpu.csr_create(3, 3, 2), gpu.csr_create(0, 0, 0)
    try:
        res = gpu.csr_from_coo_gpu(C, rows, cols, count, *bufs, gpu.CooConfig(duplicates=gpu.COO_SUM))
        assert res.error_code == 0
        got = _device_result(gpu, C, rows, cols)
        rp, ci = bc.np_coo_sum_structure(rows, cols, r, c)
        _same(got[:2], (rp, ci), ("csr_from_coo_gpu against numpy", count))
        assert gpu.csr_from_coo_cpu(H, rows, cols, r, c, v) == 0
        _same(got, gpu.csr_host_arrays(H), ("csr_from_coo_gpu against csr_from_coo_cpu", count))
        # nnz_out is the last element of the index scan
        assert res.nnz_out == ci.size == C.contents.nnz and res.combined == count - ci.size > 0
    finally:
        for buf in bufs:
            buf.release()
        gpu.csr_destroy(C)
        gpu.csr_destroy(H)


def _aggregate(gpu, n):
    _, rp, ci, va = mc.path_equal(n)
    A = _upload(gpu, n, n, (rp, ci, va))
    d_agg = _int_buffer(gpu, np.full(n, POISON))
    try:
        status, want, count, rounds = gpu.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
        assert status == 0
        status, got_count, got_rounds = gpu.amg_aggregate_mis2_gpu(A, d_agg, 0.08, 0)
        assert status == 0
        got = d_agg.copyToHost(n)
        assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
        assert got_count == count == got.max() + 1 and 1 <= got_rounds <= rounds
        # the numbers are the ranks of the roots: they grow across every tile border of the flags' scan
        assert np.all(np.diff(got.astype(np.int64)) >= 0) and got[min(n, 4096) - 1] > 0
    finally:
        d_agg.release()
        gpu.csr_destroy(A)


def _transpose(gpu, nnz):
    for passes in (1, 2, 3):
        rows, cols, (rp, ci, va) = bc.transpose_case(nnz, passes)
        A = _upload(gpu, rows, cols, (rp, ci, va))
        T = gpu.csr_create(3, 3, 2)
        try:
            assert gpu.csr_transpose_gpu(T, A) == 0
            got = _device_result(gpu, T, cols, rows)
            _same(got, bc.np_transpose(rows, cols, rp, ci, va), ("csr_transpose_gpu against numpy", nnz, passes))
        finally:
            gpu.csr_destroy(A)
            gpu.csr_destroy(T)


SCAN_CALLERS = {
    "csr_add": (_add, bc.SCAN_ROWS),
    "csr_permute_gpu": (_permute, bc.SCAN_ROWS),
    "spgemm_csr": (_product, bc.SPGEMM_ROWS),
    "fsai_csr": (_fsai, bc.FSAI_ROWS),
    "csr_from_coo_gpu": (_from_coo, bc.COO_TRIPLETS),
    "amg_aggregate_mis2_gpu": (_aggregate, bc.MIS2_ROWS),
    "csr_transpose_gpu": (_transpose, bc.TRANSPOSE_NNZ),
}
SCAN_TABLE = [(name, size) for name, (_, sizes) in SCAN_CALLERS.items() for size in sizes]


@pytest.mark.parametrize("name,size", SCAN_TABLE)
def test_every_caller_of_the_scan_on_and_around_its_tiles(gpu, name, size):
    SCAN_CALLERS[name][0](gpu, size)


def test_setup_on_the_device_reuses_the_finest_levels_scratch_below_it(gpu):
    """amg_setup_device on 8192 rows: the scan of the finest level is two tiles, the coarser ones run in the same
    scratch; every level equals amg_setup handed the definition's maps."""
    n, rp, ci, va = mc.path_equal(8192)
    cfg = gpu.AMGConfig()
    maps, _ = definition_maps(gpu, n, rp, ci, va, cfg, 0)
    assert len(maps) >= 3 and maps[0].max() + 1 > 1024
    dev, host = DeviceHier(gpu, n, rp, ci, va, cfg, 0), Hier(gpu, n, rp, ci, va, cfg, maps)
    try:
        assert dev.res.error_code == 0 and dev.H is not None and host.res.error_code == 0
        got, want = dev.levels(), host.levels()
        assert [lv["n"] for lv in got] == [lv["n"] for lv in want] == [n] + [int(m.max()) + 1 for m in maps]
        assert_levels_equal(got, want, "path_equal(8192)")
        assert dev.res.levels == host.res.levels == len(maps) + 1
    finally:
        dev.close()
        host.close()


# ---- the third level ----------------------------------------------------------------------------------------------
THIRD_LEVEL = {
    "csr_add": (_add, bc.THIRD_LEVEL_ROWS),
    "csr_permute_gpu": (_permute, bc.THIRD_LEVEL_ROWS[1:]),
    "spgemm_csr": (_product, bc.SPGEMM_THIRD_LEVEL_ROWS),
}
THIRD_LEVEL_TABLE = [(name, size) for name, (_, sizes) in THIRD_LEVEL.items() for size in sizes]


@pytest.mark.parametrize("name,size", THIRD_LEVEL_TABLE)
def test_the_scan_on_and_past_4096_squared_elements(gpu, name, size):
    """levels [16 777 216, 4096, 1] and [16 777 217, 4097, 2, 1] for csr_add and csr_permute_gpu (rows + 1 elements),
    [16 777 213, 4096, 1] and [16 777 219, 4097, 2, 1] for spgemm_csr's class scan (6 m + 1): almost every row is empty"""
    scanned = bc.SEGMENTS * size + 1 if name == "spgemm_csr" else size + 1
    assert bc.scan_depth(scanned) == (3 if scanned > bc.TILE ** 2 else 2)
    THIRD_LEVEL[name][0](gpu, size)


# ---- row_of at the workgroup edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(bc.ROW_OF_SHAPES))
def test_row_of_every_entry_where_rows_meet_the_workgroups(gpu, shape):
    lengths = bc.ROW_OF_SHAPES[shape]
    rows, nnz = lengths.size, int(lengths.sum())
    want = np.repeat(np.arange(rows, dtype=np.int32), lengths)
    # the direct door, into a view whose padding must stay as it was
    for offset, cols in ((1, 200), (2, 300)):
        rp, ci, va = bc.spread_columns(lengths, cols, 20 + nnz)
        with av.Views(gpu) as V:
            A, _ = V.csr(rows, cols, rp, ci, va, (offset, 3, 0))
            out = V.out(nnz, offset)
            assert gpu.csr_row_indices_gpu(A, out.ptr) == 0
            assert out.download().view(np.int32).tobytes() == want.tobytes(), (shape, offset)
            V.check_guards(("csr_row_indices_gpu", shape))
        # the transpose: its first pass reads row_of (one pass: from the scratch; two: from the result's columns)
        A, T = _upload(gpu, rows, cols, (rp, ci, va)), gpu.csr_create(3, 3, 2)
        assert gpu.csr_transpose_gpu(T, A) == 0
        _same(_device_result(gpu, T, cols, rows), bc.np_transpose(rows, cols, rp, ci, va), (shape, cols))
        gpu.csr_destroy(A)
        gpu.csr_destroy(T)


@pytest.mark.parametrize("shape", ["257 in one row", "257 rows of one", "513 in one row", "513 rows of one"])
def test_transpose_without_a_pass_writes_row_of_into_the_result(gpu, shape):
    lengths = bc.ROW_OF_SHAPES[shape]
    rows, nnz = lengths.size, int(lengths.sum())
    rp = bc.row_ptrs_of(lengths)
    ci, va = np.full(nnz, 4, np.int32), np.random.default_rng(nnz).uniform(-2, 2, nnz).astype(np.float32)
    A, T = _upload(gpu, rows, 7, (rp, ci, va)), gpu.csr_create(3, 3, 2)
    assert gpu.csr_transpose_gpu(T, A) == 0
    got = _device_result(gpu, T, 7, rows)
    _same(got, bc.np_transpose(rows, 7, rp, ci, va), shape)
    assert got[1].tobytes() == np.repeat(np.arange(rows, dtype=np.int32), lengths).tobytes()
    gpu.csr_destroy(A)
    gpu.csr_destroy(T)


# ---- the structure check past its grid cap ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checked(gpu):
    """regime -> (row_ptrs, cols, vals), computed once and left unchanged"""
    made = {}

    def get(regime):
        if regime not in made:
            made[regime] = bc.validate_matrix(regime)
            for a in made[regime]:
                a.setflags(write=False)
        return made[regime]
    return get


@pytest.mark.parametrize("regime", ["entries", "rows"])
def test_structure_check_finds_a_defect_on_every_trip(gpu, checked, regime):
    E = gpu.SpMVError
    rp, ci, va = checked(regime)
    rows, cols, nnz = bc.VALIDATE_ROWS, bc.VALIDATE_COLS, ci.size
    defects = bc.validate_defects(rp, ci)
    assert len(defects) == (12 if regime == "entries" else 10)
    with av.Views(gpu) as V:
        out = V.out(nnz, 1)
        clean = _upload(gpu, rows, cols, (rp, ci, va))
        assert gpu.csr_row_indices_gpu(clean, out.ptr) == 0
        assert out.download().view(np.int32).tobytes() == bc.rows_of(rp).tobytes()
        gpu.csr_destroy(clean)
        out.upload(np.full(nnz, av.SENTINEL, np.uint32).view(np.float32))
        for name, defect in defects.items():
            bad_rp, bad_ci = bc.with_defect(rp, ci, defect)
            M = _upload(gpu, rows, cols, (bad_rp, bad_ci, va))
            status = gpu.csr_row_indices_gpu(M, out.ptr)
            gpu.csr_destroy(M)
            assert status == E.INVALID_FORMAT, (regime, name, status)
        assert np.all(out.download().view(np.uint32) == av.SENTINEL)
        V.check_guards(("csr_row_indices_gpu", regime))


@pytest.mark.parametrize("name", bc.DOOR_DEFECTS)
def test_every_door_of_the_structure_check_sees_a_defect_past_the_first_trip(gpu, checked, name):
    """The matrix is rejected before any kernel follows a row pointer or a column (read in each caller: the check is
    waited for first; csr_permute_gpu's length kernel, enqueued with it, reads row pointers only)."""
    E = gpu.SpMVError
    rp, ci, va = checked("entries")
    rows, nnz = bc.VALIDATE_ROWS, ci.size
    bad_rp, bad_ci = bc.with_defect(rp, ci, bc.validate_defects(rp, ci)[name])
    M = _upload(gpu, rows, rows, (bad_rp, bad_ci, va))                     # square: four of the doors ask for it
    sentinel = np.full(max(nnz, rows), av.SENTINEL, np.uint32)
    d_out = gpu.CudaBuffer(sentinel.size, "uint32")
    d_out.copyFromHost(sentinel, sentinel.size)
    untouched = lambda: bool(np.all(d_out.copyToHost(sentinel.size) == av.SENTINEL))
    try:
        assert gpu.csr_scale_gpu(M, None, None, d_out) == E.INVALID_FORMAT and untouched()
        assert gpu.csr_diagonal_gpu(M, d_out) == E.INVALID_FORMAT and untouched()
        assert gpu.csr_color(M, d_out).error_code == E.INVALID_FORMAT and untouched()
        B = _upload(gpu, 2, 2, (np.asarray([0, 1, 2], np.int32), np.asarray([1, 0], np.int32), np.ones(2, np.float32)))
        before = (B.contents.d_row_ptrs, B.contents.d_col_indices, B.contents.d_values, B.contents.num_rows, B.contents.nnz)
        assert gpu.csr_permute_gpu(B, M) == E.INVALID_FORMAT
        assert (B.contents.d_row_ptrs, B.contents.d_col_indices, B.contents.d_values, B.contents.num_rows,
                B.contents.nnz) == before
        gpu.csr_destroy(B)
        for uplo in (0, 1):
            res = gpu.sptrsv_analyze_device(M, uplo)
            assert res.error_code == E.INVALID_FORMAT and res.num_levels == 0
            assert gpu.sptrsv_schedule_get(M, uplo)[0] == E.INVALID_ARGUMENT
        assert gpu.amg_aggregate_mis2_gpu(M, d_out, 0.08, 0) == (E.INVALID_FORMAT, -7, -7) and untouched()
        res, H = gpu.amg_setup_device(M, gpu.AMGConfig(), 0)
        assert H is None and res.error_code == E.INVALID_FORMAT
        assert gpu.csr_from_gpu(M) == 0                                    # and the matrix is as it was uploaded
        _same(gpu.csr_host_arrays(M), (bad_rp, bad_ci, va), name)
    finally:
        d_out.release()
        gpu.csr_destroy(M)


# ---- iota past its grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [3, 1])
def test_ordering_past_one_trip_of_iota(gpu, classes):
    n = bc.IOTA_ITEMS + 257
    colors = (np.arange(n) % classes).astype(np.int32)
    d_colors = _int_buffer(gpu, colors)
    d_perm, d_inverse = _int_buffer(gpu, np.full(n, POISON)), _int_buffer(gpu, np.full(n, POISON))
    status, color_ptr = gpu.color_ordering(n, d_colors, classes, d_perm, d_inverse)
    perm, inverse = d_perm.copyToHost(n), d_inverse.copyToHost(n)
    for buf in (d_colors, d_perm, d_inverse):
        buf.release()
    want = rc.ordering(colors, classes)
    assert status == 0
    _same((perm, inverse, color_ptr), want, ("color_ordering", classes))
