"""csr_transpose_gpu (include/spmv/csr_matrix.h) and spmv_csr_transpose (include/spmv/spmv.h) on the device.

The transpose is checked bit for bit against numpy's stable transpose (argsort by column, kind="stable"): row
pointers, column indices and value bits, on small shapes chosen for their edges and on the full-size generators
(involution).  y = A^T x is checked against the CPU oracle on the numpy transpose (SCALAR_CSR bit for bit, the
reordering kernels within the reordered-sum bound) and against spmv_csr on an explicit csr_transpose_gpu result
(bit for bit, every kernel type).  Also the validation, the cached transpose's lifetime, its isolation from A's
own single-vector state, the async variant and a C++ drop-in."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, reorder_err

pytestmark = pytest.mark.gpu

SCALAR, VECTOR, MERGE, ELL = 0, 1, 2, 3
TOL = 1e-5
TILED_SMALL = "min_cols=1,min_nnz=1"


# ------------------------------------------------------------------------------------------ helpers
def np_transpose(rows, cols, rp, ci, va):
    rp, ci, va = np.asarray(rp, np.int64), np.asarray(ci, np.int32), np.asarray(va, np.float32)
    perm = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    rp_t = np.zeros(cols + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=cols), out=rp_t[1:])
    return rp_t.astype(np.int32), row_of[perm], va[perm]


class Dev:
    """A CSR matrix over device arrays this object owns (csr_wrap_device), with its host arrays."""

    def __init__(self, gpu, rows, cols, rp, ci, va):
        self.gpu, self.rows, self.cols = gpu, rows, cols
        self.rp = np.asarray(rp, np.int32)
        self.ci = np.asarray(ci, np.int32)
        self.va = np.asarray(va, np.float32)
        self.nnz = int(self.ci.size)
        self.d_rp = gpu.CudaBuffer(max(self.rp.size, 1), "int32")
        self.d_ci = gpu.CudaBuffer(max(self.nnz, 1), "int32")
        self.d_va = gpu.CudaBuffer(max(self.nnz, 1), "float32")
        if self.rp.size:
            self.d_rp.copyFromHost(self.rp, self.rp.size)
        if self.nnz:
            self.d_ci.copyFromHost(self.ci, self.nnz)
            self.d_va.copyFromHost(self.va, self.nnz)
        self.A = gpu.csr_wrap_device(rows, cols, self.nnz, self.d_rp.get(), self.d_ci.get(), self.d_va.get())

    def transpose(self):
        return np_transpose(self.rows, self.cols, self.rp, self.ci, self.va)

    def close(self):
        self.gpu.csr_destroy(self.A)
        for b in (self.d_rp, self.d_ci, self.d_va):
            b.release()


def device_transpose(gpu, A):
    """(AT handle, row_ptrs, col_indices, values) of csr_transpose_gpu(A), fetched with csr_from_gpu."""
    AT = gpu.csr_create(0, 0, 0)
    status = gpu.csr_transpose_gpu(AT, A)
    assert status == 0, gpu.spmv_error_string(status)
    assert AT.contents.owns_device_memory
    assert gpu.csr_from_gpu(AT) == 0
    rp, ci, va = gpu.csr_host_arrays(AT)
    return AT, rp, ci, va


def assert_same_csr(got, want, what=""):
    for g, w, name in zip(got, want, ("row_ptrs", "col_indices", "values")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if name == "values":
            g, w = g.view(np.uint32), w.astype(np.float32).view(np.uint32)
        assert np.array_equal(g, w), (what, name, int(np.flatnonzero(g != w)[0]))


def _lens_csr(rng, lens, cols, sorted_rows=True):
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    nnz = int(rp[-1])
    ci = rng.integers(0, cols, nnz).astype(np.int32) if cols > 0 else np.zeros(0, np.int32)
    if sorted_rows:
        for r in np.flatnonzero(lens > 1):
            ci[rp[r]:rp[r + 1]] = np.sort(ci[rp[r]:rp[r + 1]])
    va = rng.uniform(-1, 1, nnz).astype(np.float32)
    return rp.astype(np.int32), ci, va


def small_shapes():
    """name -> (rows, cols, rp, ci, va)"""
    rng = np.random.default_rng(31)
    out = {}
    out["random"] = (300, 250) + _lens_csr(rng, rng.integers(0, 30, 300), 250)
    lens = rng.integers(0, 12, 200)
    lens[rng.random(200) < 0.4] = 0
    rp, ci, va = _lens_csr(rng, lens, 90)
    ci = np.where(ci % 7 == 3, ci - 1, ci).astype(np.int32)          # columns 3, 10, 17, ... stay empty
    out["empty_rows_and_columns"] = (200, 90, rp, ci, va)
    out["one_row"] = (1, 40) + _lens_csr(rng, [23], 40)
    out["one_column"] = (70, 1) + _lens_csr(rng, rng.integers(0, 3, 70), 1)
    out["rows_not_mult_64"] = (131, 77) + _lens_csr(rng, rng.integers(1, 9, 131), 77)
    lens = rng.integers(0, 8, 150)
    lens[70] = 20_000
    out["long_row"] = (150, 30_000) + _lens_csr(rng, lens, 30_000)
    out["rows_much_more_than_cols"] = (5000, 3) + _lens_csr(rng, rng.integers(0, 4, 5000), 3)
    out["cols_much_more_than_rows"] = (3, 200_000) + _lens_csr(rng, [5000, 0, 7000], 200_000)
    # duplicates and unsorted columns inside rows (a wrapped caller's arrays)
    lens = rng.integers(0, 25, 120)
    rp, ci, va = _lens_csr(rng, lens, 40, sorted_rows=False)
    starts = rp[:-1][lens >= 2]
    ci[starts + 1] = ci[starts]                          # a duplicate at the head of every row of two or more
    out["duplicates_unsorted"] = (120, 40, rp, ci, va)
    # special values: -0.0, NaN payloads, infinities, denormals, explicit zeros
    rp, ci, va = _lens_csr(rng, rng.integers(1, 10, 100), 60)
    bits = va.view(np.uint32)
    specials = np.array([0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x00000001,
                         0x807FFFFF, 0x00000000], np.uint32)
    bits[: specials.size * 20] = np.tile(specials, 20)[: min(bits.size, specials.size * 20)]
    out["special_values"] = (100, 60, rp, ci, bits.view(np.float32))
    return out


@pytest.fixture(scope="module")
def shapes(gpu):
    mats = {name: Dev(gpu, *spec) for name, spec in small_shapes().items()}
    yield mats
    for M in mats.values():
        M.close()


def _x_for(M, seed):
    return np.random.default_rng(seed).uniform(-1, 1, M.rows).astype(np.float32)


def _run_t(gpu, M, x, cfg, sentinel=True):
    d_x = gpu.CudaBuffer(max(M.rows, 1))
    if M.rows:
        d_x.copyFromHost(x, M.rows)
    d_y = gpu.CudaBuffer(max(M.cols, 1))
    if sentinel and M.cols:
        d_y.copyFromHost(np.full(M.cols, 0x7FC0DEAD, np.uint32).view(np.float32), M.cols)
    res = gpu.spmv_csr_transpose(M.A, d_x, d_y, cfg, M.rows)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    return d_y.copyToHost(M.cols).view(np.uint32).copy(), res


def _run_plain(gpu, A, rows_of_y, x, cfg):
    d_x = gpu.CudaBuffer(max(x.size, 1))
    if x.size:
        d_x.copyFromHost(x, x.size)
    d_y = gpu.CudaBuffer(max(rows_of_y, 1))
    res = gpu.spmv_csr(A, d_x, d_y, cfg, x.size)
    assert res.error_code == 0
    return d_y.copyToHost(rows_of_y).view(np.uint32).copy()


CONFIGS = {"scalar": (SCALAR, False), "vector": (VECTOR, False), "merge": (MERGE, False),
           "vector_tex": (VECTOR, True), "merge_tex": (MERGE, True)}


# ------------------------------------------------------------------------------------ structure
def test_structure_bit_for_bit_on_small_shapes(gpu, shapes):
    for name, M in shapes.items():
        AT, *got = device_transpose(gpu, M.A)
        assert (AT.contents.num_rows, AT.contents.num_cols, AT.contents.nnz) == (M.cols, M.rows, M.nnz), name
        assert_same_csr(got, M.transpose(), name)
        gpu.csr_destroy(AT)


def test_a_column_with_more_than_200k_entries(gpu):
    rng = np.random.default_rng(5)
    rows, cols = 260_000, 5000
    lens = rng.integers(0, 4, rows)
    rp, ci, va = _lens_csr(rng, lens + 1, cols)
    ci[rp[:-1]] = 7                                      # every row starts with column 7
    M = Dev(gpu, rows, cols, rp, ci, va)
    assert np.count_nonzero(ci == 7) > 200_000
    AT, *got = device_transpose(gpu, M.A)
    assert_same_csr(got, M.transpose())
    gpu.csr_destroy(AT)
    M.close()


@pytest.mark.parametrize("cols", [200, 60_000, 5_000_000, (1 << 24) + 17])
def test_one_to_four_digit_passes(gpu, cols):
    rng = np.random.default_rng(cols % 1000)
    rows = 3000
    rp, ci, va = _lens_csr(rng, rng.integers(0, 60, rows), cols)
    ci[:4] = [0, cols - 1, cols // 2, cols - 1]
    M = Dev(gpu, rows, cols, rp, ci, va)
    AT, *got = device_transpose(gpu, M.A)
    assert_same_csr(got, M.transpose(), cols)
    gpu.csr_destroy(AT)
    M.close()


def test_constant_column_skips_every_pass(gpu):
    rng = np.random.default_rng(2)
    rp, ci, va = _lens_csr(rng, rng.integers(0, 5, 400), 1)
    ci[:] = 0
    for cols in (1, 70_000):                        # all entries in column 0 of a wide matrix, too
        M = Dev(gpu, 400, cols, rp, ci, va)
        AT, *got = device_transpose(gpu, M.A)
        assert_same_csr(got, M.transpose(), cols)
        gpu.csr_destroy(AT)
        M.close()


def test_empty_edges(gpu):
    # nnz == 0: all-zero row pointers
    M = Dev(gpu, 50, 33, np.zeros(51, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    AT, rp, ci, va = device_transpose(gpu, M.A)
    assert AT.contents.nnz == 0 and np.array_equal(rp, np.zeros(34, np.int32)) and ci.size == 0
    gpu.csr_destroy(AT)
    M.close()
    # rows == 0: num_cols empty rows
    Z = gpu.csr_create(0, 12, 0)
    assert gpu.csr_to_gpu(Z) == 0
    AT, rp, ci, va = device_transpose(gpu, Z)
    assert (AT.contents.num_rows, AT.contents.num_cols) == (12, 0) and np.array_equal(rp, np.zeros(13, np.int32))
    gpu.csr_destroy(AT)
    gpu.csr_destroy(Z)
    # cols == 0: a 0-row transpose whose row_ptrs is {0}
    C = Dev(gpu, 9, 0, np.zeros(10, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    AT, rp, ci, va = device_transpose(gpu, C.A)
    assert (AT.contents.num_rows, AT.contents.num_cols) == (0, 9) and np.array_equal(rp, np.zeros(1, np.int32))
    gpu.csr_destroy(AT)
    C.close()


def test_transpose_in_place_and_from_a_host_uploaded_matrix(gpu, shapes):
    M = shapes["random"]
    A = gpu.csr_from_arrays(M.rows, M.cols, M.rp, M.ci, M.va)
    assert gpu.csr_to_gpu(A) == 0
    assert gpu.csr_transpose_gpu(A, A) == 0                  # AT may be A
    assert gpu.csr_from_gpu(A) == 0
    assert (A.contents.num_rows, A.contents.num_cols) == (M.cols, M.rows)
    assert_same_csr(gpu.csr_host_arrays(A), M.transpose())
    gpu.csr_destroy(A)


# ----------------------------------------------------------------------------------- validation
def test_invalid_input_gives_invalid_format_and_leaves_at_untouched(gpu, shapes):
    E = gpu.SpMVError
    M = shapes["random"]
    AT, *_ = device_transpose(gpu, shapes["one_row"].A)
    fields = lambda: tuple(getattr(AT.contents, f) for f in ("num_rows", "num_cols", "nnz", "d_values",
                                                             "d_col_indices", "d_row_ptrs", "owns_device_memory"))
    before = fields()
    cases = {}
    ci = M.ci.copy(); ci[17] = -1; cases["negative column"] = (M.rp, ci)
    ci = M.ci.copy(); ci[-1] = M.cols; cases["column == num_cols"] = (M.rp, ci)
    rp = M.rp.copy(); rp[40] = rp[41] + 1; cases["non-monotone"] = (rp, M.ci)
    rp = M.rp.copy(); rp[-1] -= 1; cases["wrong end"] = (rp, M.ci)
    rp = M.rp.copy(); rp[0] = 1; cases["row_ptrs[0] != 0"] = (rp, M.ci)
    for name, (rp, ci) in cases.items():
        B = Dev(gpu, M.rows, M.cols, rp, ci, M.va)
        assert gpu.csr_transpose_gpu(AT, B.A) == E.INVALID_FORMAT, name
        assert fields() == before, name
        # spmv_csr_transpose reports the build's error, writes nothing
        d_x, d_y = gpu.CudaBuffer(M.rows), gpu.CudaBuffer(M.cols)
        d_y.copyFromHost(np.full(M.cols, 0x7FC0DEAD, np.uint32).view(np.float32), M.cols)
        assert gpu.spmv_csr_transpose(B.A, d_x, d_y).error_code == E.INVALID_FORMAT, name
        assert gpu.spmv_csr_transpose_async(B.A, d_x, d_y) == E.INVALID_FORMAT, name
        assert np.all(d_y.copyToHost(M.cols).view(np.uint32) == 0x7FC0DEAD), name
        B.close()
    gpu.csr_destroy(AT)


# ---------------------------------------------------------------------------------- full size
def _involution(gpu, D):
    AT = gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(AT, D.handle) == 0
    ATT = gpu.csr_create(0, 0, 0)
    assert gpu.csr_transpose_gpu(ATT, AT) == 0
    assert gpu.csr_from_gpu(ATT) == 0
    assert_same_csr(gpu.csr_host_arrays(ATT), D.to_host())
    gpu.csr_destroy(ATT)
    return AT


def test_involution_c2_and_c4_with_spmv_parity(gpu, oracle):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    for name, D in (("C2", wl.uniform_csr_device(42, 1_000_000, 1_000_000, 16)),
                    ("C4", wl.power_law_csr_device(4, 1_000_000, 1_000_000))):
        AT = _involution(gpu, D)
        assert gpu.csr_from_gpu(AT) == 0
        rp_t, ci_t, va_t = gpu.csr_host_arrays(AT)
        rp, ci, va = D.to_host()
        assert np.array_equal(rp_t[1:] - rp_t[:-1], np.bincount(ci, minlength=D.cols)), name
        d_x = wl.vector_device(42, 3, D.rows)
        x = d_x.copyToHost(D.rows)
        want = oracle.spmv_csr(rp_t, ci_t, va_t, x)
        d_y = gpu.CudaBuffer(D.cols)
        for kernel in (SCALAR, VECTOR, MERGE):
            res = gpu.spmv_csr_transpose(D.handle, d_x, d_y, gpu.SpMVConfig(kernel), D.rows)
            assert res.error_code == 0
            got = d_y.copyToHost(D.cols)
            if kernel == SCALAR:
                np.testing.assert_array_equal(got, want, err_msg=name)
            else:
                assert reorder_err(rp_t, ci_t, va_t, x, want, got) <= TOL, (name, kernel)
        gpu.csr_destroy(AT)
        D.close()


def test_involution_c5_and_its_row_pointers(gpu):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    n = 10_000_000
    D = wl.uniform_csr_device(42, n, n, 16)
    AT = _involution(gpu, D)
    rp_t = np.empty(n + 1, np.int32)
    assert gpu.lib().spmv_c_memcpy_d2h(rp_t.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(AT.contents.d_row_ptrs),
                                       rp_t.nbytes) == 0
    ci = D.col_indices.copyToHost(D.nnz)
    want = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=n), out=want[1:])
    assert np.array_equal(rp_t, want)
    gpu.csr_destroy(AT)
    D.close()


# --------------------------------------------------------------------------------- spmv parity
def test_spmv_parity_on_small_shapes(gpu, oracle, shapes, monkeypatch):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)
    for name, M in shapes.items():
        rp_t, ci_t, va_t = M.transpose()
        x = _x_for(M, 3)
        want = oracle.spmv_csr(rp_t, ci_t, va_t, x)
        AT, *_ = device_transpose(gpu, M.A)
        for cname, (kernel, tex) in CONFIGS.items():
            cfg = gpu.SpMVConfig(kernel, 256, tex)
            bits, res = _run_t(gpu, M, x, cfg)
            got = bits.view(np.float32)
            if kernel == SCALAR:        # (NaN payloads of arithmetic results are the hardware's: compared as NaN)
                np.testing.assert_array_equal(got, want, err_msg=name)
            else:
                assert reorder_err(rp_t, ci_t, va_t, x, want, got) <= TOL, (name, cname)
            # exactly spmv_csr on the explicit transpose, and the same from run to run
            assert np.array_equal(bits, _run_plain(gpu, AT, M.cols, x, cfg)), (name, cname)
            assert np.array_equal(bits, _run_t(gpu, M, x, cfg)[0]), (name, cname)
        gpu.csr_destroy(AT)


def test_default_config_and_ell_kernel_give_the_scalar_bits(gpu, oracle, shapes):
    M = shapes["duplicates_unsorted"]
    x = _x_for(M, 4)
    want = oracle.spmv_csr(*M.transpose(), x).view(np.uint32)
    assert np.array_equal(_run_t(gpu, M, x, None)[0], want)
    assert np.array_equal(_run_t(gpu, M, x, gpu.SpMVConfig(ELL))[0], want)


def test_result_fields(gpu, shapes):
    M = shapes["random"]
    x = _x_for(M, 5)
    for kernel in (SCALAR, VECTOR, MERGE):
        _, res = _run_t(gpu, M, x, gpu.SpMVConfig(kernel))
        assert res.elapsed_ms > 0 and res.y is not None
        assert res.gflops == pytest.approx(2.0 * M.nnz / (res.elapsed_ms * 1e6), rel=1e-4)
        AT, *_ = device_transpose(gpu, M.A)
        bw = gpu.compute_bandwidth_csr(AT, res.elapsed_ms).achieved_bandwidth_gb_s
        assert res.bandwidth_gb_s == pytest.approx(bw, rel=1e-6)
        gpu.csr_destroy(AT)


def test_no_rows_or_no_entries_write_zeros_and_no_columns_writes_nothing(gpu):
    E = gpu.SpMVError
    d_x, d_y = gpu.CudaBuffer(64), gpu.CudaBuffer(64)
    for rows, cols in ((0, 40), (30, 40)):
        M = Dev(gpu, rows, cols, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        for kernel in (SCALAR, VECTOR, MERGE):
            d_y.copyFromHost(np.full(64, 0x7FC0DEAD, np.uint32).view(np.float32), 64)
            assert gpu.spmv_csr_transpose(M.A, d_x, d_y, gpu.SpMVConfig(kernel), rows).error_code == E.SUCCESS
            got = d_y.copyToHost(64).view(np.uint32)
            assert np.all(got[:cols] == 0) and np.all(got[cols:] == 0x7FC0DEAD), (rows, kernel)
        M.close()
    M = Dev(gpu, 20, 0, np.zeros(21, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    d_y.copyFromHost(np.full(64, 0x7FC0DEAD, np.uint32).view(np.float32), 64)
    assert gpu.spmv_csr_transpose(M.A, d_x, d_y, None, 20).error_code == E.SUCCESS
    assert np.all(d_y.copyToHost(64).view(np.uint32) == 0x7FC0DEAD)
    M.close()


def test_bad_block_size_is_reported_as_spmv_csr_reports_it(gpu, shapes):
    M = shapes["random"]
    bad = gpu.SpMVConfig(SCALAR, 0)
    d_x, d_y = gpu.CudaBuffer(M.rows), gpu.CudaBuffer(M.cols)
    want = gpu.spmv_csr(M.A, d_y, d_x, bad, M.cols).error_code
    assert want != 0
    assert gpu.spmv_csr_transpose(M.A, d_x, d_y, bad, M.rows).error_code == want
    assert gpu.spmv_csr_transpose_async(M.A, d_x, d_y, bad, M.rows, None) == want


# ------------------------------------------------------------------------------------- lifetime
def test_in_place_change_needs_invalidate_and_then_gives_the_new_result(gpu, oracle):
    rng = np.random.default_rng(8)
    M = Dev(gpu, 500, 300, *_lens_csr(rng, rng.integers(0, 20, 500), 300))
    x = _x_for(M, 6)
    cfg = gpu.SpMVConfig(SCALAR)
    old = _run_t(gpu, M, x, cfg)[0]
    assert np.array_equal(old, oracle.spmv_csr(*M.transpose(), x).view(np.uint32))
    M.va = (M.va * np.float32(-2.0) + np.float32(0.5)).astype(np.float32)
    M.d_va.copyFromHost(M.va, M.nnz)
    gpu.csr_invalidate_gpu_cache(M.A)
    assert np.array_equal(_run_t(gpu, M, x, cfg)[0], oracle.spmv_csr(*M.transpose(), x).view(np.uint32))
    M.close()


def test_swapped_value_array_is_noticed_without_invalidate(gpu, oracle):
    rng = np.random.default_rng(9)
    M = Dev(gpu, 400, 350, *_lens_csr(rng, rng.integers(0, 20, 400), 350))
    x = _x_for(M, 7)
    cfg = gpu.SpMVConfig(SCALAR)
    _run_t(gpu, M, x, cfg)
    va2 = rng.uniform(-3, 3, M.nnz).astype(np.float32)
    d_va2 = gpu.CudaBuffer(M.nnz)
    d_va2.copyFromHost(va2, M.nnz)
    M.A.contents.d_values = d_va2.get()
    want = oracle.spmv_csr(*np_transpose(M.rows, M.cols, M.rp, M.ci, va2), x)
    assert np.array_equal(_run_t(gpu, M, x, cfg)[0], want.view(np.uint32))
    M.A.contents.d_values = M.d_va.get()
    d_va2.release()
    M.close()


def test_two_matrices_over_one_row_pointer_array_take_turns(gpu, oracle):
    rng = np.random.default_rng(10)
    rows, cols = 600, 420
    rp, ci1, va1 = _lens_csr(rng, rng.integers(0, 15, rows), cols)
    M1 = Dev(gpu, rows, cols, rp, ci1, va1)
    ci2 = rng.integers(0, cols, ci1.size).astype(np.int32)
    va2 = rng.uniform(-1, 1, ci1.size).astype(np.float32)
    d_ci2, d_va2 = gpu.CudaBuffer(ci1.size, "int32"), gpu.CudaBuffer(ci1.size)
    d_ci2.copyFromHost(ci2, ci2.size)
    d_va2.copyFromHost(va2, va2.size)
    A2 = gpu.csr_wrap_device(rows, cols, int(ci1.size), M1.d_rp.get(), d_ci2.get(), d_va2.get())
    x = _x_for(M1, 11)
    want1 = oracle.spmv_csr(*np_transpose(rows, cols, rp, ci1, va1), x).view(np.uint32)
    want2 = oracle.spmv_csr(*np_transpose(rows, cols, rp, ci2, va2), x).view(np.uint32)
    d_x, d_y = gpu.CudaBuffer(rows), gpu.CudaBuffer(cols)
    d_x.copyFromHost(x, rows)
    for turn in range(6):
        for A, want in ((M1.A, want1), (A2, want2)):
            assert gpu.spmv_csr_transpose(A, d_x, d_y, gpu.SpMVConfig(SCALAR), rows).error_code == 0
            assert np.array_equal(d_y.copyToHost(cols).view(np.uint32), want), turn
    gpu.csr_destroy(A2)
    d_ci2.release()
    d_va2.release()
    M1.close()


def test_free_and_reupload_gives_correct_results(gpu, oracle):
    rng = np.random.default_rng(14)
    rows, cols = 700, 500
    rp, ci, va = _lens_csr(rng, rng.integers(0, 12, rows), cols)
    A = gpu.csr_from_arrays(rows, cols, rp, ci, va)
    x = rng.uniform(-1, 1, rows).astype(np.float32)
    d_x, d_y = gpu.CudaBuffer(rows), gpu.CudaBuffer(cols)
    d_x.copyFromHost(x, rows)
    want = oracle.spmv_csr(*np_transpose(rows, cols, rp, ci, va), x).view(np.uint32)
    for cycle in range(3):
        assert gpu.csr_to_gpu(A) == 0
        for kernel in (SCALAR, MERGE):
            assert gpu.spmv_csr_transpose(A, d_x, d_y, gpu.SpMVConfig(kernel), rows).error_code == 0
            got = d_y.copyToHost(cols)
            if kernel == SCALAR:
                assert np.array_equal(got.view(np.uint32), want), cycle
        gpu.csr_free_gpu(A)
        # new values between cycles, uploaded by the next csr_to_gpu
        va = (va + np.float32(1.0)).astype(np.float32)
        ctypes.memmove(A.contents.values, va.ctypes.data, va.nbytes)
        want = oracle.spmv_csr(*np_transpose(rows, cols, rp, ci, va), x).view(np.uint32)
    gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------ isolation
def test_transpose_calls_leave_a_single_vector_state_alone(gpu, oracle):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    n = 100_000
    D = wl.uniform_csr_device(8, n, n, 16)
    assert gpu.tiled_shape(D.rows, D.cols, D.nnz)[0]
    x = wl.vector_device(8, 1, n)
    y = gpu.CudaBuffer(n)
    merge = gpu.SpMVConfig(MERGE)
    assert gpu.spmv_csr(D.handle, x, y, merge, n).error_code == 0
    first = y.copyToHost(n).view(np.uint32).copy()
    before = gpu.get_tiled_promotion()
    gpu.set_tiled_promotion(4)
    try:
        for call in range(10):
            cfg = gpu.SpMVConfig(VECTOR if call % 2 else MERGE)
            assert gpu.spmv_csr_transpose(D.handle, x, y, cfg, n).error_code == 0
            assert not gpu.csr_has_tiled_plan(D.handle), call
        assert gpu.spmv_csr(D.handle, x, y, merge, n).error_code == 0
        assert np.array_equal(y.copyToHost(n).view(np.uint32), first)
        assert not gpu.csr_has_tiled_plan(D.handle)
    finally:
        gpu.set_tiled_promotion(before)
    D.close()


# ---------------------------------------------------------------------------------------- async
def test_async_on_a_side_stream_equals_the_synchronous_call(gpu, shapes, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)
    side = torch.cuda.Stream()
    for name in ("long_row", "special_values", "cols_much_more_than_rows"):
        M = shapes[name]
        x = _x_for(M, 12)
        for cname, (kernel, tex) in CONFIGS.items():
            cfg = gpu.SpMVConfig(kernel, 256, tex)
            sync_bits = _run_t(gpu, M, x, cfg)[0]
            d_x, d_y = gpu.CudaBuffer(M.rows), gpu.CudaBuffer(M.cols)
            d_x.copyFromHost(x, M.rows)
            assert gpu.spmv_csr_transpose_async(M.A, d_x, d_y, cfg, M.rows, side.cuda_stream) == 0
            side.synchronize()
            assert np.array_equal(d_y.copyToHost(M.cols).view(np.uint32), sync_bits), (name, cname)


def test_async_first_call_builds_on_its_stream(gpu, oracle):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(15)
    M = Dev(gpu, 900, 800, *_lens_csr(rng, rng.integers(0, 30, 900), 800))
    x = _x_for(M, 16)
    want = oracle.spmv_csr(*M.transpose(), x).view(np.uint32)
    side = torch.cuda.Stream()
    d_x, d_y = gpu.CudaBuffer(M.rows), gpu.CudaBuffer(M.cols)
    d_x.copyFromHost(x, M.rows)
    assert gpu.spmv_csr_transpose_async(M.A, d_x, d_y, gpu.SpMVConfig(SCALAR), M.rows, side.cuda_stream) == 0
    side.synchronize()
    assert np.array_equal(d_y.copyToHost(M.cols).view(np.uint32), want)
    M.close()


# ------------------------------------------------------------------------------------- C++ drop-in
def test_cpp_transpose_smoke(gpu, tmp_path):
    """tests/cpp/transpose_smoke.cpp through spmv/*.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "transpose_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "transpose_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
