"""How every routine that builds a CSR matrix hands its result to the output handle, for all of them in
one table.

Device builders (csr_transpose_gpu, csr_permute_gpu, csr_from_coo_gpu, spgemm_csr, csr_add, csr_diag_matrix_gpu,
fsai_csr): the handle held another, uploaded matrix with a cached transpose; afterwards it has the result's shape, owns
host and device arrays, csr_from_gpu fills the host arrays with the host twin's bits, both products on the handle are
those of the NEW matrix at zero tolerance (nothing cached for the old one survives), and the column and value arrays
are null exactly when there are no entries.  Host twins (csr_permute_cpu, csr_from_coo_cpu, spgemm_cpu_csr, csr_add_cpu,
csr_diag_matrix_cpu, fsai_cpu_csr): the device arrays are gone and the host arrays are the result."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCALAR = 0      # SpMVConfig.SCALAR_CSR: the CPU's summation order, on the transpose's rows too

# 5 x 7 with 9 entries; rows strictly ascending, an empty row, an empty column
RECT = (5, 7, np.asarray([0, 3, 3, 5, 8, 9], np.int32), np.asarray([0, 2, 6, 1, 2, 0, 3, 6, 5], np.int32),
        np.asarray([1.5, -2.0, 0.25, 3.0, -0.75, 2.5, 1.0e-3, -4.0, 7.0], np.float32))
# the second operand of the sum (5 x 7) and of the product (7 x 4)
RECT_B = (5, 7, np.asarray([0, 2, 3, 3, 5, 6], np.int32), np.asarray([2, 4, 0, 3, 4, 5], np.int32),
          np.asarray([0.5, 1.25, -3.0, 2.0, -1.5, 0.125], np.float32))
RIGHT = (7, 4, np.asarray([0, 2, 3, 5, 5, 6, 7, 9], np.int32), np.asarray([0, 3, 1, 0, 2, 3, 1, 0, 2], np.int32),
         np.asarray([2.0, -1.0, 0.5, 1.5, -2.5, 3.0, 0.75, -0.25, 4.0], np.float32))
ROW_PERM = np.asarray([3, 0, 4, 2, 1], np.int32)
COL_INVERSE = np.asarray([4, 6, 0, 2, 5, 1, 3], np.int32)


def _tridiagonal(n=6):
    """The n x n SPD matrix tridiag(-1, 4 + i / 8, -1)."""
    rows = [[(j, -1.0 if j != i else 4.0 + i / 8.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return (n, n, rp, np.asarray([c for r in rows for c, _ in r], np.int32),
            np.asarray([v for r in rows for _, v in r], np.float32))


def _empty(rows, cols):
    return rows, cols, np.zeros(rows + 1, np.int32), np.empty(0, np.int32), np.empty(0, np.float32)


def _np_transpose(rows, cols, rp, ci, va):
    perm = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    rp_t = np.zeros(cols + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=cols), out=rp_t[1:])
    return cols, rows, rp_t.astype(np.int32), row_of[perm].astype(np.int32), va[perm]


def _host(gpu, matrix):
    return gpu.csr_from_arrays(*matrix)


def _device(gpu, matrix):
    M = _host(gpu, matrix)
    assert gpu.csr_to_gpu(M) == 0
    return M


def _buffer(gpu, array, dtype):
    buf = gpu.CudaBuffer(max(array.size, 1), dtype)
    if array.size:
        buf.copyFromHost(array, array.size)
    return buf


def _result_of(gpu, M):
    m = M.contents
    return (m.num_rows, m.num_cols) + gpu.csr_host_arrays(M)


def _target(gpu):
    """A handle that holds another matrix on the host and on the device, and a cached transpose in the side table."""
    T = _device(gpu, (3, 2, np.asarray([0, 1, 1, 1], np.int32), np.asarray([1], np.int32), np.asarray([2.0], np.float32)))
    d_x, d_y = _buffer(gpu, np.ones(3, np.float32), "float32"), gpu.CudaBuffer(2)
    assert gpu.spmv_csr_transpose(T, d_x, d_y, None, 3).error_code == 0
    assert d_y.copyToHost(2).tolist() == [0.0, 2.0]
    d_x.release()
    d_y.release()
    return T


def _triplets(matrix, seed):
    rows, cols, rp, ci, va = matrix
    order = np.random.default_rng(seed).permutation(ci.size)
    return np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))[order], ci[order], va[order]


# ---- the builders: name -> (device call, host twin), both (gpu, out, case) -> status; a case is a tuple of matrices ----
def _transpose_gpu(gpu, out, case):
    A = _device(gpu, case[0])
    status = gpu.csr_transpose_gpu(out, A)
    gpu.csr_destroy(A)
    return status


def _permute(device):
    def run(gpu, out, case):
        rows, cols = case[0][0], case[0][1]
        perm, inverse = ROW_PERM[:rows], COL_INVERSE[:cols]
        if not device:
            A = _host(gpu, case[0])
            status = gpu.csr_permute_cpu(out, A, perm if rows else None, inverse if cols else None)
            gpu.csr_destroy(A)
            return status
        A = _device(gpu, case[0])
        d_perm, d_inverse = _buffer(gpu, perm, "int32"), _buffer(gpu, inverse, "int32")
        status = gpu.csr_permute_gpu(out, A, d_perm if rows else None, d_inverse if cols else None)
        d_perm.release()
        d_inverse.release()
        gpu.csr_destroy(A)
        return status
    return run


def _from_coo(device):
    def run(gpu, out, case):
        rows, cols = case[0][0], case[0][1]
        r, c, v = _triplets(case[0], 5)
        if not device:
            return gpu.csr_from_coo_cpu(out, rows, cols, r, c, v)
        bufs = [_buffer(gpu, r, "int32"), _buffer(gpu, c, "int32"), _buffer(gpu, v, "float32")]
        status = gpu.csr_from_coo_gpu(out, rows, cols, r.size, *bufs).error_code
        for buf in bufs:
            buf.release()
        return status
    return run


def _two_operands(device_call, host_call):
    def run(device):
        def call(gpu, out, case):
            A, B = ((_device if device else _host)(gpu, m) for m in case)
            status = device_call(gpu, out, A, B) if device else host_call(gpu, out, A, B)
            gpu.csr_destroy(A)
            gpu.csr_destroy(B)
            return status
        return call
    return run


_product = _two_operands(lambda gpu, C, A, B: gpu.spgemm_csr(C, A, B).error_code,
                         lambda gpu, C, A, B: gpu.spgemm_cpu_csr(C, A, B))
_sum = _two_operands(lambda gpu, C, A, B: gpu.csr_add(C, 1.5, A, -0.75, B).error_code,
                     lambda gpu, C, A, B: gpu.csr_add_cpu(C, 1.5, A, -0.75, B))


def _diag_matrix(device):
    def run(gpu, out, case):
        diag = case[0]
        if not device:
            return gpu.csr_diag_matrix_cpu(out, diag.size, diag)
        d_diag = _buffer(gpu, diag, "float32")
        status = gpu.csr_diag_matrix_gpu(out, diag.size, d_diag)
        d_diag.release()
        return status
    return run


def _fsai(device):
    def run(gpu, out, case):
        A = (_device if device else _host)(gpu, case[0])
        status = gpu.fsai_csr(out, A).error_code if device else gpu.fsai_cpu_csr(out, A)[0]
        gpu.csr_destroy(A)
        return status
    return run


BUILDERS = {
    "csr_transpose_gpu": (_transpose_gpu, None),
    "csr_permute_gpu": (_permute(True), _permute(False)),
    "csr_from_coo_gpu": (_from_coo(True), _from_coo(False)),
    "spgemm_csr": (_product(True), _product(False)),
    "csr_add": (_sum(True), _sum(False)),
    "csr_diag_matrix_gpu": (_diag_matrix(True), _diag_matrix(False)),
    "fsai_csr": (_fsai(True), _fsai(False)),
}
TWIN_NAMES = {"csr_permute_gpu": "csr_permute_cpu", "csr_from_coo_gpu": "csr_from_coo_cpu", "spgemm_csr": "spgemm_cpu_csr",
              "csr_add": "csr_add_cpu", "csr_diag_matrix_gpu": "csr_diag_matrix_cpu", "fsai_csr": "fsai_cpu_csr"}
DIAG = np.asarray([2.0, -0.5, 0.0, 1.0e-3, 7.0, -3.0e38], np.float32)

# inputs per builder: the full one, one with rows and no entries, one with no rows (where the routine takes them: a
# diagonal matrix has as many entries as rows, and fsai_csr wants a stored diagonal in every row)
CASES = {
    "csr_transpose_gpu": {"full": (RECT,), "no entries": (_empty(5, 7),), "no rows": (_empty(0, 7),)},
    "csr_permute_gpu": {"full": (RECT,), "no entries": (_empty(5, 7),), "no rows": (_empty(0, 7),)},
    "csr_from_coo_gpu": {"full": (RECT,), "no entries": (_empty(5, 7),), "no rows": (_empty(0, 7),)},
    "spgemm_csr": {"full": (RECT, RIGHT), "no entries": (_empty(5, 7), RIGHT), "no rows": (_empty(0, 7), RIGHT)},
    "csr_add": {"full": (RECT, RECT_B), "no entries": (_empty(5, 7), _empty(5, 7)), "no rows": (_empty(0, 7), _empty(0, 7))},
    "csr_diag_matrix_gpu": {"full": (DIAG,), "no rows": (DIAG[:0],)},
    "fsai_csr": {"full": (_tridiagonal(),), "no rows": (_empty(0, 0),)},
}
TABLE = [(name, case) for name in BUILDERS for case in CASES[name]]


def _expected(gpu, name, case):
    """(rows, cols, row_ptrs, col_indices, values) of the host twin on the same input."""
    if name == "csr_transpose_gpu":
        return _np_transpose(*case[0])
    H = gpu.csr_create(0, 0, 0)
    assert BUILDERS[name][1](gpu, H, case) == 0
    want = _result_of(gpu, H)
    gpu.csr_destroy(H)
    return want


def _check_handed_over(gpu, oracle, out, want, what):
    rows, cols, rp, ci, va = want
    m = out.contents
    assert (m.num_rows, m.num_cols, m.nnz) == (rows, cols, ci.size), what
    assert m.owns_host_memory and m.owns_device_memory, what
    assert m.d_row_ptrs, what
    assert (m.d_col_indices is None) == (ci.size == 0) and (m.d_values is None) == (ci.size == 0), what
    assert bool(m.col_indices) == (ci.size > 0) and bool(m.values) == (ci.size > 0) and bool(m.row_ptrs), what
    assert gpu.csr_from_gpu(out) == 0, what
    got = gpu.csr_host_arrays(out)
    for g, w, part in zip(got, (rp, ci, va), ("row_ptrs", "col_indices", "values")):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, part)
    # both products are the new matrix's: nothing cached for the old arrays answers
    rng = np.random.default_rng(11)
    x, xt = rng.uniform(-2, 2, cols).astype(np.float32), rng.uniform(-2, 2, rows).astype(np.float32)
    config = gpu.SpMVConfig(kernel_type=SCALAR)
    sentinel = np.full(max(rows, cols, 1), 0x7FC0DEAD, np.uint32).view(np.float32)
    d_x, d_xt, d_y = _buffer(gpu, x, "float32"), _buffer(gpu, xt, "float32"), gpu.CudaBuffer(sentinel.size)
    d_y.copyFromHost(sentinel, sentinel.size)
    assert gpu.spmv_csr(out, d_x, d_y, config).error_code == 0, what
    if rows:
        assert d_y.copyToHost(rows).tobytes() == oracle.spmv_csr(rp, ci, va, x).tobytes(), what
    d_y.copyFromHost(sentinel, sentinel.size)
    assert gpu.spmv_csr_transpose(out, d_xt, d_y, config).error_code == 0, what
    if cols:
        t = _np_transpose(rows, cols, rp, ci, va)
        assert d_y.copyToHost(cols).tobytes() == oracle.spmv_csr(t[2], t[3], t[4], xt).tobytes(), what
    for buf in (d_x, d_xt, d_y):
        buf.release()


@pytest.mark.parametrize("name,case", TABLE)
def test_device_builder_hands_its_arrays_to_a_handle_that_held_another_matrix(gpu, oracle, name, case):
    inputs = CASES[name][case]
    want = _expected(gpu, name, inputs)
    out = _target(gpu)
    assert BUILDERS[name][0](gpu, out, inputs) == 0
    _check_handed_over(gpu, oracle, out, want, (name, case))
    gpu.csr_destroy(out)


@pytest.mark.parametrize("case", ["full", "no entries"])
def test_transpose_into_its_own_input(gpu, oracle, case):
    matrix = RECT if case == "full" else _empty(5, 7)
    A = _device(gpu, matrix)
    d_x, d_y = _buffer(gpu, np.ones(5, np.float32), "float32"), gpu.CudaBuffer(7)
    assert gpu.spmv_csr_transpose(A, d_x, d_y, None, 5).error_code == 0     # (a cached transpose of the old A)
    d_x.release()
    d_y.release()
    assert gpu.csr_transpose_gpu(A, A) == 0
    _check_handed_over(gpu, oracle, A, _np_transpose(*matrix), ("csr_transpose_gpu(A, A)", case))
    gpu.csr_destroy(A)


def _check_host_result(gpu, out, want, what):
    rows, cols, rp, ci, va = want
    m = out.contents
    assert (m.num_rows, m.num_cols, m.nnz) == (rows, cols, ci.size), what
    assert m.d_row_ptrs is None and m.d_col_indices is None and m.d_values is None, what
    assert m.owns_host_memory, what
    for g, w, part in zip(gpu.csr_host_arrays(out), (rp, ci, va), ("row_ptrs", "col_indices", "values")):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, part)


@pytest.mark.parametrize("name", list(TWIN_NAMES))
def test_host_twin_drops_the_device_arrays_of_its_output(gpu, name):
    twin = BUILDERS[name][1]
    inputs = CASES[name]["full"]
    want = _expected(gpu, name, inputs)

    # 1. a handle that holds uploaded device arrays (and a cached transpose): they are freed, the flag goes with them
    out = _target(gpu)
    assert out.contents.owns_device_memory
    assert twin(gpu, out, inputs) == 0
    _check_host_result(gpu, out, want, (TWIN_NAMES[name], "uploaded"))
    assert not out.contents.owns_device_memory
    gpu.csr_destroy(out)

    # The two values below are what the commit before the shared hand-over produced (this test was run against it):
    # 2. a handle that never had device arrays: csr_free_gpu is not called, the flag stays as csr_create left it
    out = gpu.csr_create(3, 2, 1)
    assert twin(gpu, out, inputs) == 0
    _check_host_result(gpu, out, want, (TWIN_NAMES[name], "host only"))
    assert not out.contents.owns_device_memory
    gpu.csr_destroy(out)

    # 3. a handle that wraps device arrays it does not own: the pointers are dropped, the arrays are the caller's still
    arrays = [_buffer(gpu, np.asarray([0, 1, 1, 1], np.int32), "int32"), _buffer(gpu, np.asarray([1], np.int32), "int32"),
              _buffer(gpu, np.asarray([2.0], np.float32), "float32")]
    out = gpu.csr_wrap_device(3, 2, 1, *[b.get() for b in arrays])
    assert twin(gpu, out, inputs) == 0
    _check_host_result(gpu, out, want, (TWIN_NAMES[name], "wrapped"))
    assert not out.contents.owns_device_memory
    assert arrays[0].copyToHost(4).tolist() == [0, 1, 1, 1] and arrays[2].copyToHost(1).tolist() == [2.0]
    for buf in arrays:
        buf.release()
    gpu.csr_destroy(out)
