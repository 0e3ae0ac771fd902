"""Block CSR on the GPU (include/spmv/bsr.h) at zero tolerance: bsr_from_csr_gpu against bsr_from_csr_cpu (ints and value
bits) on every shape of tests/bsr_cases.py, at forced lane counts and past the grid cap; device validation with B
untouched; the CPU-order kernel against spmv_cpu_bsr and spmv_cpu_csr bit for bit; every lane count x every block size
on exact data against int64; random floats within the reordered-sum bound; x and y inside larger buffers; all five
arrays as views; the way back and the round trip; the values-only refill; the counting pass; a side stream; and a C++
caller."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import array_views as av
import bsr_cases as bc
import exact_data as ed
from conftest import ROOT, reorder_err

pytestmark = pytest.mark.gpu

SCALAR, VECTOR, MERGE, ELL = 0, 1, 2, 3


def _upload(gpu, m, n, arrays):
    A = gpu.csr_from_arrays(m, n, *arrays)
    assert gpu.csr_to_gpu(A) == 0
    return A


def _host_twin(gpu, A, b):
    H = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_cpu(H, A, b) == 0
    out = gpu.bsr_host_arrays(H)
    gpu.bsr_destroy(H)
    return out


def _download(gpu, B):
    assert gpu.bsr_from_gpu(B) == 0
    return gpu.bsr_host_arrays(B)


def _fields(B):
    c = B.contents
    return (c.num_rows, c.num_cols, c.block_dim, c.num_block_rows, c.num_block_cols, c.num_blocks,
            ctypes.cast(c.values, ctypes.c_void_p).value, bool(c.owns_host_memory), bool(c.owns_device_memory),
            c.d_block_row_ptrs, c.d_block_cols, c.d_values)


def _build(gpu, A, b, want, what=""):
    """bsr_from_csr_gpu against the host twin's arrays: (result, B)."""
    m, n, nnz = A.contents.num_rows, A.contents.num_cols, A.contents.nnz
    B = gpu.bsr_create(3, 3, 2, 1)
    res = gpu.bsr_from_csr_gpu(B, A, b)
    assert res.error_code == 0, (what, res.error_code)
    c = B.contents
    assert (c.num_rows, c.num_cols, c.block_dim, c.num_blocks) == (m, n, b, want[1].size), what
    assert (c.num_block_rows, c.num_block_cols) == (bc.blocks_along(m, b), bc.blocks_along(n, b))
    assert c.owns_device_memory and c.owns_host_memory
    bc.assert_same(_download(gpu, B), want, what)
    assert res.num_blocks == want[1].size and res.lanes in bc.LANES
    assert res.max_block_row == (int(np.diff(want[0]).max()) if want[0].size > 1 else 0)
    inside = bc.to_csr(m, n, b, *want, 1)[1].size
    assert res.fill == (np.float32(nnz / inside) if inside else 0.0), what
    assert res.launches >= (4 if want[1].size else 0)
    return res, B


def _vector(gpu, values, dtype="float32"):
    values = np.ascontiguousarray(values)
    buf = gpu.CudaBuffer(max(values.size, 1), dtype)
    if values.size:
        buf.copyFromHost(values, values.size)
    return buf


def _run(gpu, B, d_x, d_y, kernel, n, m):
    cfg = None if kernel is None else gpu.SpMVConfig(kernel_type=kernel)
    res = gpu.spmv_bsr(B, d_x, d_y, cfg, n)
    assert res.error_code == 0, (kernel, res.error_code)
    return d_y.copyToHost(max(m, 1))[:m]


def _device_bsr(gpu, m, n, b, brp, cols, vals):
    B = gpu.bsr_from_arrays(m, n, b, brp, cols, vals)
    assert gpu.bsr_to_gpu(B) == 0 and B.contents.owns_device_memory
    return B


# ---- 1. conversion against the host twin ---------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_conversion_and_way_back_equal_the_host_twins_on_every_shape(gpu, b):
    for name, m, n, arrays in bc.conversion_cases(b):
        A = _upload(gpu, m, n, arrays)
        want = _host_twin(gpu, A, b)
        res, B = _build(gpu, A, b, want, name)
        assert gpu.csr_block_count_gpu(A, b) == (0, want[1].size), name
        # the way back, both flags, against bsr_to_csr_cpu; the round trip drops the stored zeros and nothing else
        for keep in (1, 0):
            H, D = gpu.csr_create(0, 0, 0), gpu.csr_create(2, 2, 1)
            assert gpu.bsr_to_csr_cpu(H, B, keep) == 0 and gpu.bsr_to_csr_gpu(D, B, keep) == 0, name
            assert (D.contents.num_rows, D.contents.num_cols, D.contents.nnz) == (m, n, H.contents.nnz)
            assert D.contents.owns_device_memory and gpu.csr_from_gpu(D) == 0
            back = gpu.csr_host_arrays(D)
            bc.assert_same(back, gpu.csr_host_arrays(H), (name, "to_csr", keep))
            gpu.csr_destroy(H)
            gpu.csr_destroy(D)
        nonzero = (bc.bits(arrays[2]) & np.uint32(0x7FFFFFFF)) != 0
        row = np.repeat(np.arange(m), np.diff(arrays[0]))[nonzero]
        rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m))]).astype(np.int32)
        bc.assert_same(back, (rp, arrays[1][nonzero], arrays[2][nonzero]), (name, "round trip"))
        gpu.bsr_destroy(B)
        gpu.csr_destroy(A)


@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_forced_lane_counts_give_identical_arrays(gpu, monkeypatch, b):
    cases = {c[0]: c for c in bc.conversion_cases(b)}
    try:
        for name in ("ragged", "structured", "long block row", "4097 block rows", "specials"):
            _, m, n, arrays = cases[name]
            A = _upload(gpu, m, n, arrays)
            want = _host_twin(gpu, A, b)
            for lanes in (1, 8, 64):
                bc.forced(monkeypatch, lanes)
                res, B = _build(gpu, A, b, want, (name, lanes))
                assert res.lanes == lanes
                assert gpu.csr_block_count_gpu(A, b) == (0, want[1].size)
                gpu.bsr_destroy(B)
            gpu.csr_destroy(A)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


@pytest.mark.parametrize("lanes", [64, 8])
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_conversion_past_the_grid_cap(gpu, monkeypatch, b, lanes):
    block_rows = ed.LANE_SIZES[lanes]
    m, n, arrays = bc.many_block_rows(b, np.random.default_rng(lanes + b), block_rows)
    A = _upload(gpu, m, n, arrays)
    want = _host_twin(gpu, A, b)
    assert want[0].size == block_rows + 1 and set(np.diff(want[0]).tolist()) == {0, 1, 2}
    bc.forced(monkeypatch, lanes)
    try:
        res, B = _build(gpu, A, b, want, (b, lanes))
        assert res.lanes == lanes
        # the refill at the same lane count, past the cap as well
        assert gpu.bsr_from_csr_numeric(B, A).error_code == 0
        bc.assert_same(_download(gpu, B), want, "refill past the cap")
        gpu.bsr_destroy(B)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


# ---- 2. rejections -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_rejections_in_the_documented_order_leave_b_untouched(gpu, b):
    E = gpu.SpMVError
    rng = np.random.default_rng(300 + b)
    m, n = 5000, 40                              # three entries a row: several workgroups at the natural lane count
    good = bc.random_csr(rng, m - 1, n, 0.08)
    rows = lambda tail: bc.csr_from_rows(
        [list(zip(good[1][good[0][i]:good[0][i + 1]].tolist(), good[2][good[0][i]:good[0][i + 1]].tolist()))
         for i in range(m - 1)] + [tail])
    ok = rows([(3, 1.0), (7, 2.0), (20, 3.0)])
    nnz = ok[1].size

    def with_ptr(index, value):
        rp = ok[0].copy()
        rp[index] = value
        return rp, ok[1], ok[2]

    bad = {
        "an unsorted row": rows([(3, 1.0), (20, 2.0), (7, 3.0)]),
        "a repeated column": rows([(3, 1.0), (7, 2.0), (7, 3.0)]),
        "a column equal to n": rows([(3, 1.0), (7, 2.0), (n, 3.0)]),
        "a negative column": rows([(-1, 1.0), (7, 2.0), (20, 3.0)]),
        "row pointers that decrease": with_ptr(m - 1, int(ok[0][m - 2]) - 1),
        "a last row pointer below nnz": with_ptr(m, nnz - 1),
    }
    G = _upload(gpu, m, n, ok)
    B = gpu.bsr_create(5, 7, 3, 1)
    before = _fields(B)
    made = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_gpu(made, G, b).error_code == 0
    structure = _download(gpu, made)[:2]
    for name, arrays in bad.items():
        X = gpu.csr_from_arrays(m, n, *arrays)
        assert gpu.csr_to_gpu(X) == 0
        assert gpu.bsr_from_csr_gpu(B, X, b).error_code == E.INVALID_FORMAT, name
        assert gpu.bsr_from_csr_gpu(B, X, 5).error_code == E.INVALID_ARGUMENT, name          # the block size comes first
        assert gpu.csr_block_count_gpu(X, b) == (E.INVALID_FORMAT, -1), name
        assert _fields(B) == before, name
        if name not in ("an unsorted row", "a repeated column"):                            # (the refill needs no sorted rows)
            assert gpu.bsr_from_csr_numeric(made, X).error_code == E.INVALID_FORMAT, name
            got = _download(gpu, made)
            assert np.array_equal(got[0], structure[0]) and np.array_equal(got[1], structure[1]), name
        gpu.csr_destroy(X)
    # null arguments, an unsupported block size, a half-uploaded A
    lib = gpu.lib()
    assert lib.spmv_c_bsr_from_csr_gpu(None, G, b, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_bsr_from_csr_gpu(B, None, b, None) == E.INVALID_ARGUMENT
    for size in (0, 1, 5, 6, 7, 16, -2):
        assert gpu.bsr_from_csr_gpu(B, G, size).error_code == E.INVALID_ARGUMENT
    g = G.contents
    for half in (gpu.csr_wrap_device(m, n, nnz, g.d_row_ptrs, None, g.d_values),
                 gpu.csr_wrap_device(m, n, nnz, g.d_row_ptrs, g.d_col_indices, None),
                 gpu.csr_wrap_device(m, n, nnz, None, g.d_col_indices, g.d_values)):
        assert gpu.bsr_from_csr_gpu(B, half, b).error_code == E.INVALID_FORMAT
        assert gpu.bsr_from_csr_gpu(B, half, 9).error_code == E.INVALID_ARGUMENT
        gpu.csr_destroy(half)
    assert _fields(B) == before
    assert gpu.bsr_from_csr_gpu(B, G, b).error_code == 0 and gpu.bsr_from_csr_numeric(made, G).error_code == 0
    # BSR -> CSR validates the block structure on the device, with A untouched
    brp, cols, vals = _download(gpu, B)
    C = gpu.csr_create(2, 3, 0)
    row = int(np.flatnonzero(np.diff(brp) >= 2)[-1])
    swapped, repeated, outside = cols.copy(), cols.copy(), cols.copy()
    swapped[brp[row]:brp[row] + 2] = cols[brp[row]:brp[row] + 2][::-1]
    repeated[brp[row] + 1] = cols[brp[row]]
    outside[brp[row + 1] - 1] = bc.blocks_along(n, b)
    short = brp.copy()
    short[-1] -= 1
    for name, (p, c) in {"swapped": (brp, swapped), "repeated": (brp, repeated), "outside": (brp, outside),
                         "pointers": (short, cols)}.items():
        X = _device_bsr(gpu, m, n, b, p, c, vals)
        assert gpu.bsr_to_csr_gpu(C, X, 1) == E.INVALID_FORMAT, name
        assert (C.contents.num_rows, C.contents.num_cols, C.contents.nnz, C.contents.d_row_ptrs) == (2, 3, 0, None), name
        gpu.bsr_destroy(X)
    for M in (G, C):
        gpu.csr_destroy(M)
    for M in (B, made):
        gpu.bsr_destroy(M)


# ---- 3. the ordered product ----------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_cpu_order_kernel_has_the_bits_of_spmv_cpu_bsr_and_of_spmv_cpu_csr(gpu, b):
    rng = np.random.default_rng(400 + b)
    for m, n, density in ((2311, 1777, 0.01), (5 * b + 1, 9 * b - 1, 0.4), (b, 300 * b + 1, 0.3), (3000, b + 1, 0.5)):
        rp, ci, va = bc.random_csr(rng, m, n, density, wide=True)
        va[rng.random(va.size) < 0.05] = 0.0
        x = bc.wide_x(rng, n)
        A = _upload(gpu, m, n, (rp, ci, va))
        B = gpu.bsr_create(0, 0, 2, 0)
        assert gpu.bsr_from_csr_gpu(B, A, b).error_code == 0 and gpu.bsr_from_gpu(B) == 0
        with np.errstate(all="ignore"):
            want = gpu.spmv_cpu_bsr(B, x)
            assert np.array_equal(bc.bits(want), bc.bits(gpu.spmv_cpu_csr(A, x)))
        d_x, d_y = _vector(gpu, x), _vector(gpu, np.full(m, np.nan, np.float32))
        for kernel in (None, SCALAR, ELL):
            assert np.array_equal(bc.bits(_run(gpu, B, d_x, d_y, kernel, n, m)), bc.bits(want)), (m, n, kernel)
            d_y.copyFromHost(np.full(m, np.nan, np.float32), m)
        d_x.release()
        d_y.release()
        gpu.csr_destroy(A)
        gpu.bsr_destroy(B)


# ---- 4. the lane sweep ---------------------------------------------------------------------------------------
def _exact_run(gpu, case, b, lanes, what):
    m, n, brp, cols, vals, x = case
    want = bc.exact_product(m, n, b, brp, cols, vals, x)
    B = _device_bsr(gpu, m, n, b, brp, cols, vals)
    d_x, d_y = _vector(gpu, x), _vector(gpu, np.full(m, np.nan, np.float32))
    for kernel in (VECTOR, MERGE, SCALAR):
        first = _run(gpu, B, d_x, d_y, kernel, n, m)
        assert np.array_equal(first, want), (what, kernel, int(np.flatnonzero(first != want)[0]))
        d_y.copyFromHost(np.full(m, np.nan, np.float32), m)
        again = _run(gpu, B, d_x, d_y, kernel, n, m)
        assert np.array_equal(bc.bits(again), bc.bits(first)), (what, kernel, "second call")
    d_x.release()
    d_y.release()
    gpu.bsr_destroy(B)


@pytest.mark.parametrize("lanes", bc.LANES)
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_every_lane_count_and_block_size_equals_the_int64_result(gpu, monkeypatch, b, lanes):
    bc.forced(monkeypatch, lanes)
    try:
        _exact_run(gpu, bc.sweep_case(lanes, b), b, lanes, (b, lanes))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


@pytest.mark.parametrize("lanes", [64, 8])
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_block_rows_past_the_grid_cap_equal_the_int64_result(gpu, monkeypatch, b, lanes):
    bc.forced(monkeypatch, lanes)
    try:
        _exact_run(gpu, bc.capped_case(lanes, b), b, lanes, ("capped", b, lanes))
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)


@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_the_natural_lane_count_is_the_lane_rule_of_the_mean_blocks_per_block_row(gpu, b):
    """Without SPMV_DEBUG the build reports pick_lanes_per_row(nnz / block rows), and the product is exact."""
    case = bc.sweep_case(4, b)
    m, n, brp, cols, vals, x = case
    _exact_run(gpu, case, b, 0, ("natural", b))
    rp, ci, va = bc.to_csr(m, n, b, brp, cols, vals, 0)
    A = _upload(gpu, m, n, (rp, ci, va))
    B = gpu.bsr_create(0, 0, 2, 0)
    res = gpu.bsr_from_csr_gpu(B, A, b)
    assert res.error_code == 0 and res.lanes == ed.lanes_for(ci.size, brp.size - 1)
    bc.assert_same(_download(gpu, B), (brp, cols, vals), "exact matrix through the build")
    gpu.csr_destroy(A)
    gpu.bsr_destroy(B)


# ---- 5. random floats ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_every_kernel_within_the_reordered_sum_bound_on_random_floats(gpu, b):
    rng = np.random.default_rng(500 + b)
    for m, n, density in ((4001, 3001, 0.004), (300, 4000 * b + 1, 0.02)):
        rp, ci, va = bc.random_csr(rng, m, n, density)
        x = rng.uniform(-2, 2, n).astype(np.float32)
        A = _upload(gpu, m, n, (rp, ci, va))
        B = gpu.bsr_create(0, 0, 2, 0)
        assert gpu.bsr_from_csr_gpu(B, A, b).error_code == 0
        prod = va.astype(np.float64) * x.astype(np.float64)[ci]
        want = np.zeros(m)
        np.add.at(want, np.repeat(np.arange(m), np.diff(rp)), prod)
        d_x, d_y = _vector(gpu, x), _vector(gpu, np.zeros(m, np.float32))
        for kernel in (SCALAR, VECTOR, MERGE, ELL, None):
            got = _run(gpu, B, d_x, d_y, kernel, n, m)
            err = reorder_err(rp, ci, va, x, want, got)
            print("b", b, "shape", (m, n), "kernel", kernel, "err", err)
            assert err < 1e-5, (kernel, err)
        d_x.release()
        d_y.release()
        gpu.csr_destroy(A)
        gpu.bsr_destroy(B)


# ---- 6. the edges of the arrays ------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_x_is_not_read_past_num_cols_and_y_is_not_written_past_num_rows(gpu, b):
    rng = np.random.default_rng(600 + b)
    m, n = 7 * b - 1, 9 * b + 1
    lens = [9, 3, 0, 10, 1, 5, 10]
    brp, cols, vals, x = bc.exact_bsr(rng, b, m, n, lens)
    assert m % b and n % b and cols.max() == bc.blocks_along(n, b) - 1 and lens[-1] > 0
    want = bc.exact_product(m, n, b, brp, cols, vals, x)
    B = _device_bsr(gpu, m, n, b, brp, cols, vals)
    d_x = _vector(gpu, np.concatenate([x, np.full(3 * b, np.nan, np.float32)]))
    canary = np.full(m + 3 * b, 12345.0, np.float32)
    d_y = _vector(gpu, canary)
    for kernel in (SCALAR, VECTOR):
        d_y.copyFromHost(canary, canary.size)
        assert gpu.spmv_bsr(B, d_x, d_y, gpu.SpMVConfig(kernel_type=kernel), n).error_code == 0
        got = d_y.copyToHost(canary.size)
        assert np.array_equal(got[:m], want), kernel                        # exact, so free of NaN
        assert np.array_equal(got[m:], canary[m:]), kernel
    # no blocks at all: zeros into y[0, m), nothing behind it; no rows: nothing is written
    E = gpu.bsr_create(m, n, b, 0)
    assert gpu.bsr_to_gpu(E) == 0
    for kernel in (SCALAR, VECTOR):
        d_y.copyFromHost(canary, canary.size)
        assert gpu.spmv_bsr(E, d_x, d_y, gpu.SpMVConfig(kernel_type=kernel), n).error_code == 0
        got = d_y.copyToHost(canary.size)
        assert not got[:m].any() and np.array_equal(got[m:], canary[m:])
    Z = gpu.bsr_wrap_device(0, n, b, 0, None, None, None)
    d_y.copyFromHost(canary, canary.size)
    assert gpu.spmv_bsr(Z, d_x, d_y, None, n).error_code == 0 and np.array_equal(d_y.copyToHost(canary.size), canary)
    for M in (B, E, Z):
        gpu.bsr_destroy(M)
    d_x.release()
    d_y.release()


@pytest.mark.parametrize("offsets", ed.VIEW_OFFSETS)
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_all_five_arrays_as_views_into_larger_buffers(gpu, b, offsets):
    rng = np.random.default_rng(700 + b + 10 * sum(offsets))
    m, n = 40 * b - 1, 37 * b + 1
    lens = rng.integers(0, 12, size=40)
    lens[[3, 17]] = [30, 0]
    brp, cols, vals, x = bc.exact_bsr(rng, b, m, n, lens)
    want = bc.exact_product(m, n, b, brp, cols, vals, x)
    with av.Views(gpu) as V:
        v_rp = V.view(brp, offsets[0], np.int32(cols.size))
        v_bc = V.view(cols, offsets[1], np.int32(bc.blocks_along(n, b) - 1))
        v_bv = V.view(vals, offsets[2], np.float32(ed.VIEW_POISON))
        v_x = V.x(x, offsets[1])
        v_y = V.out(m, offsets[2])
        B = gpu.bsr_wrap_device(m, n, b, cols.size, v_rp.ptr, v_bc.ptr, v_bv.ptr)
        assert B is not None and not B.contents.owns_device_memory
        for kernel in (SCALAR, VECTOR):
            v_y.upload(np.full(m, av.SENTINEL, np.uint32).view(np.float32))
            assert gpu.spmv_bsr(B, v_x.ptr, v_y.ptr, gpu.SpMVConfig(kernel_type=kernel), n).error_code == 0
            V.check_guards((b, offsets, kernel))
            assert np.array_equal(v_y.download(), want), (b, offsets, kernel)
        # the way back from the views, and the refill into them
        C = gpu.csr_create(0, 0, 0)
        assert gpu.bsr_to_csr_gpu(C, B, 0) == 0 and gpu.csr_from_gpu(C) == 0
        bc.assert_same(gpu.csr_host_arrays(C), bc.to_csr(m, n, b, brp, cols, vals, 0), "views, to_csr")
        A, _ = V.csr(m, n, *gpu.csr_host_arrays(C), offsets)
        v_bv.upload(np.full(vals.size, 3.0, np.float32))
        assert gpu.bsr_from_csr_numeric(B, A).error_code == 0
        V.check_guards((b, offsets, "refill"))
        assert np.array_equal(bc.bits(v_bv.download()), bc.bits(vals))
        assert np.array_equal(v_rp.download(), brp) and np.array_equal(v_bc.download(), cols)
        built = gpu.bsr_create(0, 0, 2, 0)
        assert gpu.bsr_from_csr_gpu(built, A, b).error_code == 0
        V.check_guards((b, offsets, "build"))
        bc.assert_same(_download(gpu, built), (brp, cols, vals), "build from views")
        gpu.bsr_destroy(built)
        gpu.csr_destroy(C)
        gpu.bsr_destroy(B)


# ---- 7. the refill -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_values_only_refill(gpu, b):
    E = gpu.SpMVError
    rng = np.random.default_rng(800 + b)
    m, n = 523, 389
    rp, ci, va = bc.random_csr(rng, m, n, 0.05)
    A = _upload(gpu, m, n, (rp, ci, va))
    B = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_gpu(B, A, b).error_code == 0
    brp, cols, vals = _download(gpu, B)
    pointers = (B.contents.d_block_row_ptrs, B.contents.d_block_cols, B.contents.d_values)
    # new values, with every entry of the first and the last block now an explicit zero
    row = np.repeat(np.arange(m), np.diff(rp))
    I = np.repeat(np.arange(brp.size - 1), np.diff(brp))
    va2 = bc.with_specials(rng, (rp, ci, (va * np.float32(-1.5) + np.float32(0.25)).astype(np.float32)))[2]
    for p in (0, cols.size - 1):
        va2[(row // b == I[p]) & (ci // b == cols[p])] = 0.0
    A2 = _upload(gpu, m, n, (rp, ci, va2))
    res = gpu.bsr_from_csr_numeric(B, A2)
    assert res.error_code == 0 and res.launches == 1 and res.num_blocks == cols.size and res.symbolic_ms == 0.0
    assert (B.contents.d_block_row_ptrs, B.contents.d_block_cols, B.contents.d_values) == pointers
    got = _download(gpu, B)
    fresh = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_gpu(fresh, A2, b).error_code == 0
    bc.assert_same(got, _download(gpu, fresh), "refill against a fresh build")
    assert got[1].size == cols.size and not bc.bits(got[2][:b * b]).any() and not bc.bits(got[2][-b * b:]).any()
    # an A with fewer entries: the blocks nobody touches stay stored, all zero
    keep = ~((row // b == I[1]) & (ci // b == cols[1]))
    rp3 = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=m))]).astype(np.int32)
    A3 = _upload(gpu, m, n, (rp3, ci[keep], va[keep]))
    assert gpu.bsr_from_csr_numeric(B, A3).error_code == 0
    got = _download(gpu, B)
    want = vals.copy()
    want[b * b:2 * b * b] = 0.0
    bc.assert_same(got, (brp, cols, want), "a block that lost its entries")
    # one entry outside B's pattern
    dense = np.zeros((bc.blocks_along(m, b), bc.blocks_along(n, b)), bool)
    dense[I, cols] = True
    Ib, Jb = [int(v[0]) for v in np.nonzero(~dense[:m // b, :n // b])]
    rows = [list(zip(ci[rp[i]:rp[i + 1]].tolist(), va[rp[i]:rp[i + 1]].tolist())) for i in range(m)]
    rows[Ib * b + b - 1] = sorted(rows[Ib * b + b - 1] + [(Jb * b, 1.0)])
    A4 = _upload(gpu, m, n, bc.csr_from_rows(rows))
    assert gpu.bsr_from_csr_numeric(B, A4).error_code == E.INVALID_FORMAT
    got = _download(gpu, B)
    assert np.array_equal(got[0], brp) and np.array_equal(got[1], cols)
    assert gpu.bsr_from_csr_numeric(B, A).error_code == 0
    bc.assert_same(_download(gpu, B), (brp, cols, vals), "the first values again")
    for M in (A, A2, A3, A4):
        gpu.csr_destroy(M)
    for M in (B, fresh):
        gpu.bsr_destroy(M)


# ---- 8. a side stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.BLOCK_DIMS)
def test_async_on_a_side_stream_has_the_synchronous_bits(gpu, b):
    torch = pytest.importorskip("torch")
    side = torch.cuda.Stream()
    rng = np.random.default_rng(900 + b)
    m, n = 3001, 2003
    rp, ci, va = bc.random_csr(rng, m, n, 0.01)
    x = rng.uniform(-2, 2, n).astype(np.float32)
    A = _upload(gpu, m, n, (rp, ci, va))
    B = gpu.bsr_create(0, 0, 2, 0)
    assert gpu.bsr_from_csr_gpu(B, A, b).error_code == 0
    d_x, d_y = _vector(gpu, x), _vector(gpu, np.zeros(m, np.float32))
    for kernel in (SCALAR, VECTOR):
        sync = _run(gpu, B, d_x, d_y, kernel, n, m)
        d_y.copyFromHost(np.full(m, np.nan, np.float32), m)
        assert gpu.spmv_bsr_async(B, d_x, d_y, gpu.SpMVConfig(kernel_type=kernel), n, side.cuda_stream) == 0
        side.synchronize()
        assert np.array_equal(bc.bits(d_y.copyToHost(m)), bc.bits(sync)), kernel
    d_x.release()
    d_y.release()
    gpu.csr_destroy(A)
    gpu.bsr_destroy(B)


# ---- 9. a C++ caller -----------------------------------------------------------------------------------------
def test_cpp_bsr_smoke(gpu):
    """tests/cpp/bsr_smoke.cpp through spmv/bsr.h, bsr_matrix.h and CudaBuffer, compiled by __graft_entry__.build()."""
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "bsr_smoke")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
