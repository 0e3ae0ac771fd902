"""csr_add / csr_add_numeric, csr_scale_gpu, csr_diagonal_gpu and csr_diag_matrix_gpu (include/spmv/csr_ops.h) on the GPU,
at zero tolerance against their host twins: row pointers, columns and value bits (NaNs by position).  Every lane
count over every row shape and overlap form; a second trip of the row sweep; a hub row; random and rectangular pairs
with special values; the triplet re-assembly route; symmetrising; the values-only pass, its pattern check and its
cache invalidation; device validation; empty results; A + A; array views; exact integers; scaling; the diagonal in
and out; and a C++ caller."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import csr_ops_cases as oc
import exact_data as ed
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILED_SMALL = "min_cols=1,min_nnz=1"


def _upload(gpu, rows, cols, arrays):
    M = gpu.csr_from_arrays(rows, cols, *arrays)
    assert gpu.csr_to_gpu(M) == 0
    return M


def _download(gpu, C):
    assert gpu.csr_from_gpu(C) == 0
    return gpu.csr_host_arrays(C)


def _put(gpu, address, array):
    array = np.ascontiguousarray(array)
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(address), array.ctypes.data_as(ctypes.c_void_p), array.nbytes) == 0


def _buffer(gpu, array, dtype="float32"):
    array = np.ascontiguousarray(array)
    buf = gpu.CudaBuffer(max(array.size, 1), dtype)
    if array.size:
        buf.copyFromHost(array, array.size)
    return buf


def _host(gpu, alpha, A, beta, B):
    C = gpu.csr_create(0, 0, 0)
    assert gpu.csr_add_cpu(C, alpha, A, beta, B) == 0
    want = gpu.csr_host_arrays(C)
    gpu.csr_destroy(C)
    return want


def _fields(C):
    m = C.contents
    return (m.num_rows, m.num_cols, m.nnz, bool(m.owns_device_memory), m.d_row_ptrs, m.d_col_indices, m.d_values)


def _sum(gpu, alpha, A, beta, B, want=None, what=""):
    """csr_add against csr_add_cpu on the same matrices: (result, C's arrays)."""
    want = _host(gpu, alpha, A, beta, B) if want is None else want
    C = gpu.csr_create(3, 3, 2)
    res = gpu.csr_add(C, alpha, A, beta, B)
    assert res.error_code == 0, (what, res.error_code)
    m = C.contents
    assert (m.num_rows, m.num_cols, m.nnz) == (A.contents.num_rows, A.contents.num_cols, want[1].size)
    assert m.owns_device_memory
    got = _download(gpu, C)
    gpu.csr_destroy(C)
    oc.assert_same(got, want, what)
    assert res.nnz == want[1].size and res.common == A.contents.nnz + B.contents.nnz - res.nnz
    assert res.max_row_nnz == (int(np.diff(want[0]).max()) if want[0].size > 1 else 0)
    assert res.launches >= (3 if res.nnz else 2) and res.lanes in oc.LANES
    return res, got


def _pair(gpu, m, n, a, b):
    return _upload(gpu, m, n, a), _upload(gpu, m, n, b)


def _forced(monkeypatch, lanes):
    if lanes:
        monkeypatch.setenv("SPMV_DEBUG", f"add_lanes={lanes}")
    else:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


# ---- 1. every lane count -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", list(oc.LANES) + [0])
def test_every_lane_count_over_every_row_shape(gpu, monkeypatch, lanes):
    n = 3_000_001
    L = lanes if lanes else 16
    a, b = oc.lane_rows(L, n, seed=40 + L)
    m = a[0].size - 1
    assert a[1].min() == 0 and a[1].max() == n - 1 and b[1].min() == 0 and b[1].max() == n - 1
    A, B = _pair(gpu, m, n, a, b)
    _forced(monkeypatch, lanes)
    try:
        res, got = _sum(gpu, 1.5, A, -0.75, B, None, f"lanes {lanes}")
        assert res.lanes == (lanes if lanes else ed.lanes_for(a[1].size + b[1].size, m))
        common = oc.common_per_row(a, b)
        assert res.common == int(common.sum())
        assert res.max_row_nnz == int((np.diff(a[0]) + np.diff(b[0]) - common).max())
        # and the values-only pass at the same lane count
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_add(C, 1.0, A, 1.0, B).error_code == 0
        again = gpu.csr_add_numeric(C, 1.5, A, -0.75, B)
        assert again.error_code == 0 and again.lanes == res.lanes and again.launches == 1
        oc.assert_same(_download(gpu, C), got, f"numeric, lanes {lanes}")
        gpu.csr_destroy(C)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- 2. past one trip of the row sweep -----------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [64, 1])
def test_second_trip_of_the_row_sweep(gpu, monkeypatch, lanes):
    m = 2 * (256 // lanes) * 2048 + 3
    rng = np.random.default_rng(50 + lanes)
    a, b = oc.short_rows(rng, m), oc.short_rows(rng, m)
    A, B = _pair(gpu, m, 64, a, b)
    _forced(monkeypatch, lanes)
    try:
        res, _ = _sum(gpu, 2.0, A, 0.5, B, None, f"second trip, lanes {lanes}")
        assert res.lanes == lanes and 0 < res.common < a[1].size
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- 3. a hub ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hub(gpu):
    rng = np.random.default_rng(60)
    n, m, at = 400_000, 41, 17
    pool = np.sort(rng.choice(n, size=95_000, replace=False))
    shared, only_a, only_b = pool[:50_000:2], pool[50_000:], pool[1:50_000:2]
    assert shared.size == 25_000 and only_a.size == 45_000 and only_b.size == 25_000
    hub_a, hub_b = np.sort(np.concatenate([shared, only_a])), np.sort(np.concatenate([shared, only_b]))
    short_a, short_b = oc.random_csr(rng, m, 50, 0.1), oc.random_csr(rng, m, 50, 0.1)

    def with_hub(short, cols):
        rows = [list(zip(short[1][short[0][i]:short[0][i + 1]].tolist(), short[2][short[0][i]:short[0][i + 1]].tolist()))
                for i in range(m)]
        rows[at] = list(zip(cols.tolist(), rng.uniform(-2, 2, cols.size).astype(np.float32).tolist()))
        return oc.csr_from_rows(rows)

    a, b = with_hub(short_a, hub_a), with_hub(short_b, hub_b)
    A, B = _pair(gpu, m, n, a, b)
    yield A, B, _host(gpu, -1.25, A, 3.0, B)
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


@pytest.mark.parametrize("lanes", [1, 64, 0])
def test_a_hub_row_between_short_rows(gpu, monkeypatch, hub, lanes):
    A, B, want = hub
    _forced(monkeypatch, lanes)
    try:
        res, _ = _sum(gpu, -1.25, A, 3.0, B, want, f"hub, lanes {lanes}")
        assert res.max_row_nnz == 95_000 and res.common >= 25_000
        if lanes:
            assert res.lanes == lanes
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


@pytest.mark.parametrize("lanes", [1, 8, 32])
def test_rows_on_both_sides_of_the_long_row_threshold(gpu, monkeypatch, lanes):
    """Rows of LONG_TILES * L - 1 ... + 2 entries in A and B together, neighbours in one wavefront, between short rows:
    the ones past the threshold are walked by the whole wavefront, several of them per wavefront, the last row of
    the matrix among them (the groups behind it have no row)."""
    rng = np.random.default_rng(90 + lanes)
    edge, n = oc.LONG_TILES * lanes, 20_000
    totals = [3, edge - 1, edge, edge + 1, edge + 2, 0, 5 * edge + 3, 1, edge + 1] * 3 + [2 * edge + 1]
    a_rows, b_rows = [], []
    for i, total in enumerate(totals):
        la = total // 2 if i % 2 else total - total // 3
        pos = oc.overlap_positions(oc.OVERLAPS[i % len(oc.OVERLAPS)], la, total - la) or \
            oc.overlap_positions("interleaved", la, total - la)
        union, inverse = np.unique(np.concatenate(pos), return_inverse=True)
        cols = np.sort(rng.choice(n, size=union.size, replace=False))
        ca, cb = cols[inverse[:la]], cols[inverse[la:]]
        a_rows.append(list(zip(ca.tolist(), rng.uniform(-3, 3, ca.size).astype(np.float32).tolist())))
        b_rows.append(list(zip(cb.tolist(), rng.uniform(-3, 3, cb.size).astype(np.float32).tolist())))
    a, b = oc.csr_from_rows(a_rows), oc.csr_from_rows(b_rows)
    lengths = np.diff(a[0]) + np.diff(b[0])
    assert lengths.tolist() == totals and (lengths > edge).sum() >= 10 and (lengths == edge).sum() == 3
    A, B = _pair(gpu, len(totals), n, a, b)
    _forced(monkeypatch, lanes)
    try:
        res, got = _sum(gpu, 0.5, A, -2.0, B, None, f"threshold, lanes {lanes}")
        assert res.lanes == lanes and res.common > 0
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_add(C, 1.0, A, 1.0, B).error_code == 0
        assert gpu.csr_add_numeric(C, 0.5, A, -2.0, B).error_code == 0
        oc.assert_same(_download(gpu, C), got, f"threshold, numeric, lanes {lanes}")
        gpu.csr_destroy(C)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- 4. random pairs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(211, 97), (97, 211), (1, 5000), (3000, 2), (64, 64)])
def test_random_pairs_rectangular_with_special_values(gpu, shape):
    m, n = shape
    rng = np.random.default_rng(m * 7 + n)
    for density_a, density_b in ((0.02, 0.3), (0.3, 0.02), (0.5, 0.5), (0.0, 0.2), (1.0, 1.0)):
        a = oc.with_specials(rng, oc.random_csr(rng, m, n, density_a))
        b = oc.with_specials(rng, oc.random_csr(rng, m, n, density_b))
        A, B = _pair(gpu, m, n, a, b)
        for alpha, beta in ((1.0, 1.0), (0.0, -1.0), tuple(float(v) for v in rng.uniform(-3, 3, 2))):
            _sum(gpu, alpha, A, beta, B, None, (shape, density_a, density_b, alpha, beta))
        gpu.csr_destroy(A)
        gpu.csr_destroy(B)


# ---- 5. against the route that exists without csr_add --------------------------------------------------------
def test_equals_the_reassembly_of_the_concatenated_triplets(gpu):
    rng = np.random.default_rng(70)
    m, n = 700, 450
    a = oc.with_specials(rng, oc.random_csr(rng, m, n, 0.05), 0.02)
    b = oc.with_specials(rng, oc.random_csr(rng, m, n, 0.08), 0.02)
    for arrays in (a, b):                        # (a NaN from an addition has one spelling there, any here: none)
        arrays[2][np.isinf(arrays[2])] = 1.0
    A, B = _pair(gpu, m, n, a, b)
    _, got = _sum(gpu, 1.0, A, 1.0, B)
    rows = np.concatenate([np.repeat(np.arange(m, dtype=np.int32), np.diff(x[0])) for x in (a, b)])
    d_rows, d_cols = _buffer(gpu, rows, "int32"), _buffer(gpu, np.concatenate([a[1], b[1]]), "int32")
    d_vals = _buffer(gpu, np.concatenate([a[2], b[2]]))
    T = gpu.csr_create(0, 0, 0)
    assert gpu.csr_from_coo_gpu(T, m, n, rows.size, d_rows, d_cols, d_vals).error_code == 0
    oc.assert_same(got, _download(gpu, T), "triplet route")
    for buf in (d_rows, d_cols, d_vals):
        buf.release()
    for M in (A, B, T):
        gpu.csr_destroy(M)


# ---- 6. symmetrising -----------------------------------------------------------------------------------------
def test_half_a_plus_half_a_transposed_is_symmetric_bit_for_bit(gpu):
    rng = np.random.default_rng(71)
    n = 300
    a = oc.random_csr(rng, n, n, 0.04)
    A = _upload(gpu, n, n, a)
    AT, S, ST = gpu.csr_create(0, 0, 0), gpu.csr_create(0, 0, 0), gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(AT, A) == 0
    assert gpu.csr_add(S, 0.5, A, 0.5, AT).error_code == 0
    assert gpu.csr_transpose_gpu(ST, S) == 0
    s, st = _download(gpu, S), _download(gpu, ST)
    oc.assert_same(s, st, "S against S^T")
    assert s[1].size > a[1].size                                        # the union, not A's pattern
    for M in (A, AT, S, ST):
        gpu.csr_destroy(M)


# ---- 7. csr_add_numeric --------------------------------------------------------------------------------------
def test_numeric_pass_alone_has_the_bits_of_a_fresh_sum_and_writes_no_structure(gpu):
    rng = np.random.default_rng(72)
    m, n = 523, 389
    a, b = oc.random_csr(rng, m, n, 0.06), oc.random_csr(rng, m, n, 0.04)
    A, B = _pair(gpu, m, n, a, b)
    first = gpu.csr_create(0, 0, 0)
    assert gpu.csr_add(first, 1.0, A, 1.0, B).error_code == 0
    rp, ci, va = _download(gpu, first)
    gpu.csr_destroy(first)
    # new values in both matrices, new alpha and beta
    a2 = (a[0], a[1], oc.with_specials(rng, (a[0], a[1], a[2] * np.float32(0.5) + np.float32(0.125)))[2])
    b2 = (b[0], b[1], (b[2] * np.float32(-3.0)).astype(np.float32))
    _put(gpu, A.contents.d_values, a2[2])
    _put(gpu, B.contents.d_values, b2[2])
    status, want = oc.host_sum(gpu, m, n, -0.375, a2, 2.5, b2)
    assert status == 0
    with av.Views(gpu) as V:
        C, (v_rp, v_ci, v_va) = V.csr(m, n, rp, ci, va, (1, 3, 2))
        res = gpu.csr_add_numeric(C, -0.375, A, 2.5, B)
        assert res.error_code == 0 and res.nnz == ci.size and res.launches == 1 and res.symbolic_ms == 0.0
        V.check_guards("csr_add_numeric")
        assert v_rp.download().tobytes() == rp.tobytes() and v_ci.download().tobytes() == ci.tobytes()
        oc.assert_same((rp, ci, v_va.download()), want, "numeric alone")
    fresh = gpu.csr_create(0, 0, 0)
    assert gpu.csr_add(fresh, -0.375, A, 2.5, B).error_code == 0
    oc.assert_same(_download(gpu, fresh), want, "fresh")
    for M in (A, B, fresh):
        gpu.csr_destroy(M)


def test_numeric_pass_alone_rejects_every_kind_of_wrong_pattern(gpu):
    E = gpu.SpMVError
    rng = np.random.default_rng(73)
    m, n = 300, 200
    a, b = oc.random_csr(rng, m, n, 0.05), oc.random_csr(rng, m, n, 0.05)
    A, B = _pair(gpu, m, n, a, b)
    rp, ci, va = _host(gpu, 1.0, A, 1.0, B)
    row = next(i for i in range(m - 1, 0, -1) if 1 < rp[i + 1] - rp[i] < n and rp[i] > rp[i - 1])
    p = int(rp[row])                                                    # the row's first entry
    absent = int(np.setdiff1d(np.arange(n), ci[rp[row]:rp[row + 1]])[0])

    def shifted(delta):
        out = rp.copy()
        out[row + 1:] += delta
        return out

    replaced = ci.copy()
    replaced[p] = absent
    moved = rp.copy()
    moved[row] -= 1                                                     # the row takes the last entry of the row above
    patterns = {
        "the pattern itself": (rp, ci, 0),
        "a column missing": (shifted(-1), np.delete(ci, p), E.INVALID_FORMAT),
        "a column added": (shifted(1), np.insert(ci, rp[row + 1], absent), E.INVALID_FORMAT),
        "a column replaced": (rp, replaced, E.INVALID_FORMAT),
        "the row boundary moved by one": (moved, ci, E.INVALID_FORMAT),
    }
    for name, (c_rp, c_ci, expect) in patterns.items():
        C = _upload(gpu, m, n, (c_rp, c_ci, np.zeros(c_ci.size, np.float32)))
        assert gpu.csr_add_numeric(C, 1.0, A, 1.0, B).error_code == expect, name
        if expect == 0:
            oc.assert_same(_download(gpu, C), (rp, ci, va), name)
        gpu.csr_destroy(C)
    for shape in ((m + 1, n), (m, n + 1), (m - 1, n)):
        W = gpu.csr_wrap_device(shape[0], shape[1], ci.size, A.contents.d_row_ptrs, A.contents.d_col_indices,
                                A.contents.d_values)
        assert gpu.csr_add_numeric(W, 1.0, A, 1.0, B).error_code == E.INVALID_DIMENSION
        gpu.csr_destroy(W)
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


# ---- 8. the cache --------------------------------------------------------------------------------------------
def _mass_and_stiffness(side):
    """M (a 3-point mass matrix per grid line) and K (the 5-point Laplacian) on a side x side grid: M + dt K is SPD."""
    n = side * side
    idx = lambda i, j: i * side + j
    m_rows, k_rows = [], []
    for i in range(side):
        for j in range(side):
            mr, kr = {idx(i, j): 4.0 / 6.0}, {idx(i, j): 4.0}
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if 0 <= i + di < side and 0 <= j + dj < side:
                    kr[idx(i + di, j + dj)] = -1.0
                    if di == 0:
                        mr[idx(i, j + dj)] = 1.0 / 6.0
            m_rows.append(sorted(mr.items()))
            k_rows.append(sorted(kr.items()))
    return n, oc.csr_from_rows(m_rows), oc.csr_from_rows(k_rows)


def test_values_only_refill_and_in_place_scaling_drop_what_was_cached(gpu, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)                       # the tiled engine also for a matrix this small
    n, mass, stiff = _mass_and_stiffness(24)
    M, K = _pair(gpu, n, n, mass, stiff)
    rng = np.random.default_rng(74)
    b = rng.standard_normal(n).astype(np.float32)
    d_b, d_x = _buffer(gpu, b), _buffer(gpu, np.zeros(n, np.float32))
    config = gpu.CGConfig(tolerance=1e-6, max_iterations=500, preconditioner=1, engine=1)

    def solve(A):
        d_x.copyFromHost(np.zeros(n, np.float32), n)
        r = gpu.cg_solve(A, d_b, d_x, config)
        assert r.error_code == 0 and r.converged
        return d_x.copyToHost(n), (r.iterations, r.relative_residual, r.converged, r.breakdown)

    def fresh(dt):
        status, arrays = oc.host_sum(gpu, n, n, 1.0, mass, dt, stiff)
        assert status == 0
        F = _upload(gpu, n, n, arrays)
        out = solve(F)
        gpu.csr_destroy(F)
        return out

    try:
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_add(C, 1.0, M, 0.01, K).error_code == 0
        x1, r1 = solve(C)
        want1 = fresh(0.01)
        assert x1.tobytes() == want1[0].tobytes() and r1 == want1[1]
        assert gpu.csr_has_tiled_plan(C)
        assert gpu.csr_add_numeric(C, 1.0, M, 0.5, K).error_code == 0
        assert not gpu.csr_has_tiled_plan(C)
        x2, r2 = solve(C)
        want2 = fresh(0.5)
        assert x2.tobytes() == want2[0].tobytes() and r2 == want2[1]
        assert x2.tobytes() != x1.tobytes()

        # in-place scaling, then the tiled SpMV
        tiled = gpu.SpMVConfig(kernel_type=gpu.SpMVConfig.VECTOR_CSR, use_texture=True)
        d_y = _buffer(gpu, np.zeros(n, np.float32))
        assert gpu.spmv_csr(C, d_b, d_y, tiled, n).error_code == 0 and gpu.csr_has_tiled_plan(C)
        before = d_y.copyToHost(n)
        scale = rng.uniform(0.5, 2.0, n).astype(np.float32)
        d_s = _buffer(gpu, scale)
        assert gpu.csr_scale_gpu(C, d_s, d_s, None) == 0
        assert not gpu.csr_has_tiled_plan(C)
        assert gpu.spmv_csr(C, d_b, d_y, tiled, n).error_code == 0
        after = d_y.copyToHost(n)
        status, arrays = oc.host_sum(gpu, n, n, 1.0, mass, 0.5, stiff)
        H = gpu.csr_from_arrays(n, n, *arrays)
        status, scaled = gpu.csr_scale_cpu(H, scale, scale)
        gpu.csr_destroy(H)
        F = _upload(gpu, n, n, (arrays[0], arrays[1], scaled))
        assert gpu.spmv_csr(F, d_b, d_y, tiled, n).error_code == 0
        assert after.tobytes() == d_y.copyToHost(n).tobytes() and after.tobytes() != before.tobytes()
        gpu.csr_destroy(F)
        for buf in (d_b, d_x, d_y, d_s):
            buf.release()
        for A in (M, K, C):
            gpu.csr_destroy(A)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


# ---- 9. device validation ------------------------------------------------------------------------------------
def test_device_validation_in_the_last_row_leaves_c_untouched(gpu):
    E = gpu.SpMVError
    rng = np.random.default_rng(75)
    m, n = 5000, 40                              # three entries a row: several workgroups at the natural lane count
    good = oc.random_csr(rng, m - 1, n, 0.08)
    last = [(3, 1.0), (7, 2.0), (20, 3.0)]
    rows = lambda tail: oc.csr_from_rows(
        [list(zip(good[1][good[0][i]:good[0][i + 1]].tolist(), good[2][good[0][i]:good[0][i + 1]].tolist()))
         for i in range(m - 1)] + [tail])
    ok = rows(last)
    nnz = ok[1].size

    def with_ptr(index, value):
        rp = ok[0].copy()
        rp[index] = value
        return rp, ok[1], ok[2]

    bad = {
        "a row out of order": rows([(3, 1.0), (20, 2.0), (7, 3.0)]),
        "a repeated column": rows([(3, 1.0), (7, 2.0), (7, 3.0)]),
        "a column equal to n": rows([(3, 1.0), (7, 2.0), (n, 3.0)]),
        "a row pointer that decreases": with_ptr(m - 1, int(ok[0][m - 2]) - 1),
        "a last row pointer below nnz": with_ptr(m, nnz - 1),
    }
    G = _upload(gpu, m, n, ok)
    C = gpu.csr_create(2, 3, 1)
    before = _fields(C)
    made = gpu.csr_create(0, 0, 0)
    assert gpu.csr_add(made, 1.0, G, 1.0, G).error_code == 0
    for name, arrays in bad.items():
        X = gpu.csr_from_arrays(m, n, *arrays)
        assert gpu.csr_to_gpu(X) == 0
        for first, second in ((X, G), (G, X), (X, X)):
            assert gpu.csr_add(C, 1.0, first, 1.0, second).error_code == E.INVALID_FORMAT, name
            assert _fields(C) == before, name
            assert gpu.csr_add_numeric(made, 1.0, first, 1.0, second).error_code == E.INVALID_FORMAT, name
        gpu.csr_destroy(X)
    assert gpu.csr_add_numeric(made, 1.0, G, 1.0, G).error_code == 0
    for M in (G, C, made):
        gpu.csr_destroy(M)


# ---- 10, 11. empty results, A is B ---------------------------------------------------------------------------
def test_empty_results(gpu):
    some = oc.csr_from_rows([[(1, 1.0)], [], [(0, -0.0), (3, 2.0)], [], [(3, np.inf)]])
    cases = {
        "m = 0": (0, 4, oc.empty(0), oc.empty(0)),
        "n = 0": (5, 0, oc.empty(5), oc.empty(5)),
        "m = n = 0": (0, 0, oc.empty(0), oc.empty(0)),
        "both empty": (5, 4, oc.empty(5), oc.empty(5)),
    }
    for name, (m, n, a, b) in cases.items():
        A, B = _pair(gpu, m, n, a, b)
        res, (rp, ci, va) = _sum(gpu, 2.0, A, 3.0, B, None, name)
        assert res.nnz == 0 and ci.size == 0 and rp.tolist() == [0] * (m + 1), name
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_add(C, 1.0, A, 1.0, B).error_code == 0
        assert gpu.csr_add_numeric(C, 2.0, A, 3.0, B).error_code == 0, name
        for M in (A, B, C):
            gpu.csr_destroy(M)
    # one empty: C is the other, scaled
    A, B = _pair(gpu, 5, 4, some, oc.empty(5))
    for alpha, beta, first, second in ((0.5, 7.0, A, B), (7.0, 0.5, B, A)):
        _, got = _sum(gpu, alpha, first, beta, second, None, "one empty")
        with np.errstate(all="ignore"):
            oc.assert_same(got, (some[0], some[1], some[2] * np.float32(0.5)), "one empty")
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)


def test_a_is_b_gives_twice_a(gpu):
    rng = np.random.default_rng(76)
    a = oc.with_specials(rng, oc.random_csr(rng, 400, 300, 0.05))
    A = _upload(gpu, 400, 300, a)
    res, got = _sum(gpu, 1.0, A, 1.0, A, None, "A + A")
    with np.errstate(all="ignore"):
        oc.assert_same(got, (a[0], a[1], a[2] * np.float32(2.0)), "2 A")
    assert res.common == a[1].size
    gpu.csr_destroy(A)


# ---- 12. views -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(1, 2, 3), (3, 1, 2)])
def test_inputs_that_are_views_into_larger_buffers(gpu, offsets):
    rng = np.random.default_rng(77)
    m, n = 161, 243
    a, b = oc.random_csr(rng, m, n, 0.1), oc.random_csr(rng, m, n, 0.07)
    status, want = oc.host_sum(gpu, m, n, 0.75, a, -1.5, b)
    assert status == 0
    with av.Views(gpu) as V:
        A, _ = V.csr(m, n, *a, offsets)
        B, _ = V.csr(m, n, *b, offsets[::-1])
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_add(C, 0.75, A, -1.5, B).error_code == 0
        V.check_guards(("csr_add", offsets))
        oc.assert_same(_download(gpu, C), want, "views")
        assert gpu.csr_add_numeric(C, 0.75, A, -1.5, B).error_code == 0
        V.check_guards(("csr_add_numeric", offsets))
        oc.assert_same(_download(gpu, C), want, "views, numeric")
        r, c = V.x(rng.uniform(-2, 2, m), offsets[0]), V.x(rng.uniform(-2, 2, n), offsets[1])
        out = V.out(a[1].size, offsets[2])
        d = V.out(m, offsets[1])
        H = gpu.csr_from_arrays(m, n, *a)
        assert gpu.csr_scale_gpu(A, r.ptr, c.ptr, out.ptr) == 0 and gpu.csr_diagonal_gpu(A, d.ptr) == 0
        V.check_guards(("csr_scale_gpu, csr_diagonal_gpu", offsets))
        assert oc.bits(out.download()).tolist() == oc.bits(gpu.csr_scale_cpu(H, r.download(), c.download())[1]).tolist()
        assert oc.bits(d.download()).tolist() == oc.bits(gpu.csr_diagonal_cpu(H)[1]).tolist()
        gpu.csr_destroy(H)
        gpu.csr_destroy(C)


# ---- 13. integers --------------------------------------------------------------------------------------------
def test_spmv_on_2a_minus_4b_equals_the_int64_result(gpu):
    rng = np.random.default_rng(78)
    m, n = 900, 300
    a, b = oc.integer_csr(rng, m, n, 0.05), oc.integer_csr(rng, m, n, 0.05)
    x = rng.integers(-64, 65, size=n).astype(np.float32)
    A, B = _pair(gpu, m, n, a, b)
    C = gpu.csr_create(0, 0, 0)
    assert gpu.csr_add(C, 2.0, A, -4.0, B).error_code == 0
    c = _download(gpu, C)
    ed.check_exact(*c, x)
    want = 2 * ed.exact_reference(*a, x).astype(np.int64) - 4 * ed.exact_reference(*b, x).astype(np.int64)
    d_x, d_y = _buffer(gpu, x), _buffer(gpu, np.zeros(m, np.float32))
    for kernel in (gpu.SpMVConfig.SCALAR_CSR, gpu.SpMVConfig.VECTOR_CSR):
        assert gpu.spmv_csr(C, d_x, d_y, gpu.SpMVConfig(kernel_type=kernel), n).error_code == 0
        np.testing.assert_array_equal(d_y.copyToHost(m).astype(np.int64), want)
    d_x.release()
    d_y.release()
    for M in (A, B, C):
        gpu.csr_destroy(M)


# ---- 14. scaling ---------------------------------------------------------------------------------------------
def test_scale_against_the_host_in_place_and_out_of_place(gpu):
    E = gpu.SpMVError
    rng = np.random.default_rng(79)
    m, n = 2311, 1777
    a = oc.with_specials(rng, oc.random_csr(rng, m, n, 0.07, sort=False, duplicates=True), 0.05)
    nnz = a[1].size
    assert nnz > ed.VEC_TRIP                     # more entries than one trip of the element-wise grid
    r, c = rng.uniform(-2, 2, m).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)
    d_r, d_c, d_out = _buffer(gpu, r), _buffer(gpu, c), _buffer(gpu, np.zeros(nnz, np.float32))
    H = gpu.csr_from_arrays(m, n, *a)
    for use_r, use_c in ((True, True), (True, False), (False, True), (False, False)):
        status, want = gpu.csr_scale_cpu(H, r if use_r else None, c if use_c else None)
        assert status == 0
        A = _upload(gpu, m, n, a)
        assert gpu.csr_scale_gpu(A, d_r if use_r else None, d_c if use_c else None, d_out) == 0
        oc.assert_same((a[0], a[1], d_out.copyToHost(nnz)), (a[0], a[1], want), ("out of place", use_r, use_c))
        oc.assert_same(_download(gpu, A), a, "A itself untouched")
        for out in (None, A.contents.d_values):                              # both spellings of in place
            _put(gpu, A.contents.d_values, a[2])
            assert gpu.csr_scale_gpu(A, d_r if use_r else None, d_c if use_c else None, out) == 0
            oc.assert_same(_download(gpu, A), (a[0], a[1], want), ("in place", use_r, use_c))
        gpu.csr_destroy(A)
    # overlaps, with real arrays
    A = _upload(gpu, m, n, a)
    values = A.contents.d_values
    assert gpu.csr_scale_gpu(A, d_r, d_c, values + 4) == E.INVALID_ARGUMENT
    assert gpu.csr_scale_gpu(A, d_r, d_c, d_r) == E.INVALID_ARGUMENT
    assert gpu.csr_scale_gpu(A, d_r, d_c, d_c.get() + 4 * (n - 1)) == E.INVALID_ARGUMENT
    assert gpu.csr_scale_gpu(A, values + 4 * (nnz - 1), d_c, None) == E.INVALID_ARGUMENT
    oc.assert_same(_download(gpu, A), a, "rejected calls write nothing")
    # a malformed structure is found on the device before anything is written
    X = gpu.csr_from_arrays(m, n, a[0], np.where(np.arange(nnz) == nnz - 1, n, a[1]), a[2])
    assert gpu.csr_to_gpu(X) == 0
    assert gpu.csr_scale_gpu(X, d_r, d_c, None) == E.INVALID_FORMAT
    assert gpu.csr_diagonal_gpu(X, d_out) == E.INVALID_FORMAT
    assert _download(gpu, X)[2].tobytes() == a[2].tobytes()                  # the values are untouched
    for M in (A, X, H):
        gpu.csr_destroy(M)
    for buf in (d_r, d_c, d_out):
        buf.release()


def test_scaling_a_symmetric_matrix_by_one_vector_keeps_it_symmetric_bit_for_bit(gpu):
    rng = np.random.default_rng(80)
    n = 500
    half = oc.random_csr(rng, n, n, 0.02)
    H = _upload(gpu, n, n, half)
    HT, S = gpu.csr_create(0, 0, 0), gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(HT, H) == 0 and gpu.csr_add(S, 1.0, H, 1.0, HT).error_code == 0
    d = rng.uniform(0.1, 3.0, n).astype(np.float32)
    d_d = _buffer(gpu, d)
    assert gpu.csr_scale_gpu(S, d_d, d_d, None) == 0
    ST = gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(ST, S) == 0
    oc.assert_same(_download(gpu, S), _download(gpu, ST), "D S D against its transpose")
    d_d.release()
    for M in (H, HT, S, ST):
        gpu.csr_destroy(M)


# ---- 15. the diagonal in and out -----------------------------------------------------------------------------
def test_diagonal_and_diag_matrix_against_the_host_and_a_shifted_matrix(gpu):
    E = gpu.SpMVError
    rng = np.random.default_rng(81)
    for m, n in ((700, 700), (900, 400), (400, 900)):
        a = oc.random_csr(rng, m, n, 0.01, sort=False, duplicates=True)
        a[1][a[0][:-1][np.diff(a[0]) > 0]] = np.flatnonzero(np.diff(a[0]) > 0) % n      # a diagonal in most rows
        A = _upload(gpu, m, n, a)
        d_d = _buffer(gpu, np.full(m, 7.0, np.float32))
        assert gpu.csr_diagonal_gpu(A, d_d) == 0
        status, want = gpu.csr_diagonal_cpu(A)
        got = d_d.copyToHost(m)
        assert status == 0 and oc.bits(got).tolist() == oc.bits(want).tolist()
        assert np.count_nonzero(got) > 100 and (m <= n or not got[n:].any())
        d_d.release()
        gpu.csr_destroy(A)
    # the vector in, the matrix out, and back
    n = ed.VEC_TRIP + 3                          # past one trip of the element-wise grid
    v = rng.uniform(-3, 3, n).astype(np.float32)
    v[[0, 5, n - 1]] = [0.0, np.inf, 1e-45]
    d_v, d_back = _buffer(gpu, v), _buffer(gpu, np.zeros(n, np.float32))
    D, HD = gpu.csr_create(3, 2, 1), gpu.csr_create(0, 0, 0)
    assert gpu.csr_diag_matrix_gpu(D, n, d_v) == 0 and gpu.csr_diag_matrix_cpu(HD, n, v) == 0
    assert (D.contents.num_rows, D.contents.num_cols, D.contents.nnz) == (n, n, n) and D.contents.owns_device_memory
    oc.assert_same(_download(gpu, D), gpu.csr_host_arrays(HD), "diag matrix")
    assert gpu.csr_diagonal_gpu(D, d_back) == 0
    assert oc.bits(d_back.copyToHost(n)).tolist() == oc.bits(v).tolist()
    assert gpu.csr_diag_matrix_gpu(D, 5, None) == 0
    assert _download(gpu, D)[2].tolist() == [1.0] * 5 and _download(gpu, D)[0].tolist() == list(range(6))
    assert gpu.csr_diag_matrix_gpu(D, 0, None) == 0 and D.contents.nnz == 0 and _download(gpu, D)[0].tolist() == [0]
    assert gpu.csr_diag_matrix_gpu(D, -1, None) == E.INVALID_DIMENSION and D.contents.num_rows == 0
    for buf in (d_v, d_back):
        buf.release()
    # A - sigma I from the pieces
    n = 800
    a = oc.random_csr(rng, n, n, 0.01)
    A = _upload(gpu, n, n, a)
    eye, HI = gpu.csr_create(0, 0, 0), gpu.csr_create(0, 0, 0)
    assert gpu.csr_diag_matrix_gpu(eye, n, None) == 0 and gpu.csr_diag_matrix_cpu(HI, n, None) == 0
    res, got = _sum(gpu, 1.0, A, -0.3, eye, _host(gpu, 1.0, A, -0.3, HI), "A - sigma I")
    assert res.nnz == a[1].size + n - res.common and got[1].size >= n
    for M in (A, eye, HI, D, HD):
        gpu.csr_destroy(M)


# ---- 16. a C++ caller ----------------------------------------------------------------------------------------
def test_cpp_csr_ops_smoke(gpu, tmp_path):
    """tests/cpp/csr_ops_smoke.cpp through spmv/csr_ops.h, csr_matrix.h and CudaBuffer, compiled here with build()'s
    g++ line."""
    exe = str(tmp_path / "csr_ops_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "csr_ops_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
