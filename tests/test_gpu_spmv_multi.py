"""spmv_csr_multi (include/spmv/spmv.h): Y = A * X for k right-hand sides, X / Y row-major with leading dimensions.
The checker is the CPU oracle applied column by column: SCALAR_CSR bit for bit, VECTOR_CSR / MERGE_PATH within the
reordered-sum bound.  Also the call's contract (padding columns, argument errors, determinism), its isolation from
the single-vector paths (promotion, merge-path state), the async variant and 64-bit offsets into X and Y."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, max_rel_err, reorder_err

pytestmark = pytest.mark.gpu

SCALAR, VECTOR, MERGE, ELL = 0, 1, 2, 3
KS = (1, 2, 3, 4, 5, 7, 8, 16, 17, 32, 33, 64)
TOL = 1e-5
SENTINEL = np.uint32(0x7FC0DEAD)       # a NaN bit pattern no kernel produces by arithmetic


def _leading_dims(k):
    return sorted({k, k + 3, (k + 3) // 4 * 4})


class Host:
    """A host-built CSR matrix copied to the device, with its host arrays for the oracle."""

    def __init__(self, spmv, rows, cols, rp, ci, va):
        self.rows, self.cols = rows, cols
        self.rp, self.ci, self.va = (np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(va, np.float32))
        self.spmv = spmv
        self.A = spmv.csr_from_arrays(rows, cols, self.rp, self.ci, self.va)
        assert spmv.csr_to_gpu(self.A) == 0

    def close(self):
        self.spmv.csr_destroy(self.A)


def _shapes(spmv):
    rng = np.random.default_rng(2024)
    out = {}
    lens = rng.integers(0, 30, 300)
    out["random"] = (300, 250, lens, 250)
    lens = rng.integers(0, 12, 200)
    lens[rng.random(200) < 0.4] = 0
    out["empty_rows"] = (200, 90, lens, 90)
    out["one_row"] = (1, 40, np.array([17]), 40)
    out["rows_not_mult_64"] = (131, 77, rng.integers(1, 9, 131), 77)
    lens = rng.integers(0, 8, 150)
    lens[70] = 20_000
    out["long_row"] = (150, 30_000, lens, 30_000)
    mats = {}
    for name, (rows, cols, lens, ncols) in out.items():
        rp, ci, va = spmv.synth.stratified_csr(11, 0, lens, ncols)
        mats[name] = Host(spmv, rows, cols, rp, ci, va)
    return mats


def _run(gpu, M, X, k, ldx, ldy, kernel):
    """X: host array (cols, ldx).  Returns Y (rows, ldy) as uint32 bits and as float32."""
    d_x = gpu.CudaBuffer(max(X.size, 1))
    d_x.copyFromHost(X.reshape(-1), X.size)
    Y0 = np.full(M.rows * ldy, SENTINEL, np.uint32)
    d_y = gpu.CudaBuffer(max(Y0.size, 1))
    d_y.copyFromHost(Y0.view(np.float32), Y0.size)
    cfg = None if kernel is None else gpu.SpMVConfig(kernel)
    res = gpu.spmv_csr_multi(M.A, d_x, d_y, k, ldx, ldy, cfg, M.cols)
    assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
    bits = d_y.copyToHost(Y0.size).view(np.uint32).reshape(M.rows, ldy)
    return bits, res


def _oracle_cols(oracle, M, X, k):
    return [oracle.spmv_csr(M.rp, M.ci, M.va, np.ascontiguousarray(X[:, j])) for j in range(k)]


def _x(rng, cols, ldx, special=False, nonneg=False):
    X = rng.uniform(-1, 1, (cols, ldx)).astype(np.float32)
    if nonneg:
        X = np.abs(X)
    if special and cols > 8:
        X[3, :] = np.inf
        X[5, ::2] = np.nan
        X[7, 1::3] = -np.inf
    return X


def _check(bits, want, k, kernel, M, X):
    Y = bits.view(np.float32)
    assert np.all(bits[:, k:] == SENTINEL), "padding columns written"
    for j in range(k):
        got = Y[:, j]
        if kernel == SCALAR:
            np.testing.assert_array_equal(got, want[j], err_msg=f"column {j}")
        else:
            err = reorder_err(M.rp, M.ci, M.va, X[:, j], want[j], got)
            assert err <= TOL, (j, err)


@pytest.fixture(scope="module")
def shapes(gpu):
    mats = _shapes(gpu)
    yield mats
    for M in mats.values():
        M.close()


@pytest.mark.parametrize("kernel", [SCALAR, VECTOR, MERGE])
def test_parity_every_k_and_leading_dimension(gpu, oracle, shapes, kernel):
    rng = np.random.default_rng(kernel)
    for name, M in shapes.items():
        for k in KS:
            for ldx in _leading_dims(k):
                X = _x(rng, M.cols, ldx, special=(name == "random" and k in (3, 8, 33)))
                want = _oracle_cols(oracle, M, X, k)
                for ldy in _leading_dims(k):
                    bits, _ = _run(gpu, M, X, k, ldx, ldy, kernel)
                    _check(bits, want, k, kernel, M, X)


@pytest.mark.parametrize("kernel", [VECTOR, MERGE])
def test_reordering_kernels_on_non_negative_data_hold_plain_relative_error(gpu, oracle, shapes, kernel):
    rng = np.random.default_rng(7)
    for name in ("random", "long_row"):
        M = shapes[name]
        va = np.abs(M.va)
        P = Host(gpu, M.rows, M.cols, M.rp, M.ci, va)
        for k in (2, 8, 17):
            X = _x(rng, M.cols, k, nonneg=True)
            want = _oracle_cols(oracle, P, X, k)
            bits, _ = _run(gpu, P, X, k, k, k, kernel)
            Y = bits.view(np.float32)
            for j in range(k):
                assert max_rel_err(want[j], Y[:, j]) <= TOL, (name, k, j)
        P.close()


def test_default_config_and_ell_kernel_give_the_scalar_bits(gpu, oracle, shapes):
    rng = np.random.default_rng(3)
    M = shapes["random"]
    for k in (1, 5, 8):
        X = _x(rng, M.cols, k + 3)
        scalar, _ = _run(gpu, M, X, k, k + 3, k, SCALAR)
        default, _ = _run(gpu, M, X, k, k + 3, k, None)
        ell, _ = _run(gpu, M, X, k, k + 3, k, ELL)
        assert np.array_equal(scalar, default) and np.array_equal(scalar, ell)


def test_two_calls_of_each_kernel_give_identical_bits(gpu, shapes):
    rng = np.random.default_rng(5)
    M = shapes["long_row"]
    for kernel in (SCALAR, VECTOR, MERGE):
        for k in (3, 8, 33):
            X = _x(rng, M.cols, k)
            a, _ = _run(gpu, M, X, k, k, k, kernel)
            b, _ = _run(gpu, M, X, k, k, k, kernel)
            assert np.array_equal(a, b), (kernel, k)


def test_result_fields(gpu, shapes):
    M = shapes["random"]
    X = _x(np.random.default_rng(1), M.cols, 8)
    for kernel in (SCALAR, VECTOR, MERGE):
        _, res = _run(gpu, M, X, 8, 8, 8, kernel)
        assert res.elapsed_ms > 0 and res.y is not None
        assert res.gflops == pytest.approx(2.0 * M.rp[-1] * 8 / (res.elapsed_ms * 1e6), rel=1e-4)
        bw = gpu.compute_bandwidth_csr_multi(M.A, 8, res.elapsed_ms).achieved_bandwidth_gb_s
        assert res.bandwidth_gb_s == pytest.approx(bw, rel=1e-6)


def test_c2_size_matrix_at_k_8(gpu, oracle):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    n, k = 1_000_000, 8
    A = wl.uniform_csr_device(42, n, n, 16)
    rp, ci, va = A.to_host()
    d_x = wl.vector_device(42, 9, n * k)
    X = d_x.copyToHost(n * k).reshape(n, k)
    want = [oracle.spmv_csr(rp, ci, va, np.ascontiguousarray(X[:, j])) for j in range(k)]
    d_y = gpu.CudaBuffer(n * k)
    for kernel in (SCALAR, VECTOR, MERGE):
        res = gpu.spmv_csr_multi(A.handle, d_x, d_y, k, config=gpu.SpMVConfig(kernel), vec_size=n)
        assert res.error_code == 0
        Y = d_y.copyToHost(n * k).reshape(n, k)
        for j in range(k):
            if kernel == SCALAR:
                np.testing.assert_array_equal(Y[:, j], want[j])
            else:
                assert reorder_err(rp, ci, va, X[:, j], want[j], Y[:, j]) <= TOL, (kernel, j)
    A.close()


def test_power_law_matrix_at_k_8_and_32(gpu, oracle):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    n = 200_000
    A = wl.power_law_csr_device(4, n, n)
    rp, ci, va = A.to_host()
    for k in (8, 32):
        d_x = wl.vector_device(4, k, n * k)
        X = d_x.copyToHost(n * k).reshape(n, k)
        want = [oracle.spmv_csr(rp, ci, va, np.ascontiguousarray(X[:, j])) for j in range(k)]
        d_y = gpu.CudaBuffer(n * k)
        for kernel in (SCALAR, VECTOR, MERGE):
            assert gpu.spmv_csr_multi(A.handle, d_x, d_y, k, config=gpu.SpMVConfig(kernel)).error_code == 0
            Y = d_y.copyToHost(n * k).reshape(n, k)
            for j in range(k):
                if kernel == SCALAR:
                    np.testing.assert_array_equal(Y[:, j], want[j])
                else:
                    assert reorder_err(rp, ci, va, X[:, j], want[j], Y[:, j]) <= TOL, (kernel, k, j)
    A.close()


# ------------------------------------------------------------------------------------------ contract
def test_empty_matrix_zeroes_exactly_the_k_columns(gpu):
    rows, cols, k, ldy = 70, 40, 5, 9
    M = Host(gpu, rows, cols, np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    X = np.ones((cols, k), np.float32)
    for kernel in (SCALAR, VECTOR, MERGE):
        bits, _ = _run(gpu, M, X, k, k, ldy, kernel)
        assert np.all(bits[:, :k] == 0) and np.all(bits[:, k:] == SENTINEL)
    M.close()


def test_zero_rows_writes_nothing(gpu):
    A = gpu.csr_create(0, 10, 0)
    d_x, d_y = gpu.CudaBuffer(40), gpu.CudaBuffer(8)
    d_y.copyFromHost(np.full(8, SENTINEL, np.uint32).view(np.float32), 8)
    for k in (4, 0, -3):
        assert gpu.spmv_csr_multi(A, d_x, d_y, k).error_code == 0
    assert np.all(d_y.copyToHost(8).view(np.uint32) == SENTINEL)
    gpu.csr_destroy(A)


def test_argument_errors_in_the_stated_order(gpu, shapes):
    E = gpu.SpMVError
    M = shapes["random"]
    k, cols, rows = 4, M.cols, M.rows
    d_x, d_y = gpu.CudaBuffer(cols * k), gpu.CudaBuffer(rows * k)
    call = lambda A=M.A, x=d_x, y=d_y, kk=k, ldx=k, ldy=k, cfg=None, vs=cols: \
        gpu.spmv_csr_multi(A, x, y, kk, ldx, ldy, cfg, vs).error_code
    # 1. nulls (before everything else)
    assert call(A=None, kk=0, vs=1) == E.INVALID_ARGUMENT
    assert call(x=0, kk=0) == E.INVALID_ARGUMENT and call(y=0, kk=0) == E.INVALID_ARGUMENT
    # 2. zero rows before k
    Z = gpu.csr_create(0, cols, 0)
    assert call(A=Z, kk=0, vs=7) == E.SUCCESS
    gpu.csr_destroy(Z)
    # 3. k before vec_size and leading dimensions
    assert call(kk=0, vs=cols + 1, ldx=-1) == E.INVALID_ARGUMENT
    # 4. / 5. vec_size, then ldx / ldy (both INVALID_DIMENSION), before the format check
    assert call(vs=cols + 1) == E.INVALID_DIMENSION
    assert call(ldx=k - 1) == E.INVALID_DIMENSION and call(ldy=k - 1) == E.INVALID_DIMENSION
    H = gpu.csr_create(3, cols, 0)                      # host-only: no device arrays
    assert call(A=H, ldx=k - 1, vs=-1) == E.INVALID_DIMENSION
    # 6. missing device arrays before the overlap check
    assert call(A=H, y=d_x, vs=-1) == E.INVALID_FORMAT
    gpu.csr_destroy(H)
    # 7. overlapping X and Y before the block size
    bad_block = gpu.SpMVConfig(0, 0)
    assert call(y=d_x) == E.INVALID_ARGUMENT
    assert call(y=d_x, cfg=bad_block) == E.INVALID_ARGUMENT
    assert call(y=d_x.get() + 4 * (cols * k - 1)) == E.INVALID_ARGUMENT      # last element of X = first of Y
    # 8. block size: as spmv_csr
    assert call(cfg=bad_block) == E.KERNEL_LAUNCH
    assert gpu.spmv_csr(M.A, d_x, d_y, bad_block, cols).error_code == E.KERNEL_LAUNCH
    # X and Y in one allocation, side by side: fine
    both = gpu.CudaBuffer(cols * (k + 2) + rows * k)
    assert call(x=both, y=both.get() + 4 * cols * k) == E.SUCCESS
    # the padding of X's last row is not part of its used range
    assert call(x=both, y=both.get() + 4 * ((cols - 1) * (k + 2) + k), ldx=k + 2) == E.SUCCESS


# ----------------------------------------------------------------------------------------- isolation
def test_multi_calls_never_build_a_tiled_plan_or_count_toward_promotion(gpu, oracle):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    n, k = 100_000, 4
    A = wl.uniform_csr_device(8, n, n, 16)
    assert gpu.tiled_shape(A.rows, A.cols, A.nnz)[0]
    d_x = wl.vector_device(8, 1, n * k)
    d_y = gpu.CudaBuffer(n * k)
    before = gpu.get_tiled_promotion()
    gpu.set_tiled_promotion(4)
    try:
        for call in range(10):
            cfg = gpu.SpMVConfig(VECTOR, 256, call % 2 == 1)        # use_texture is ignored
            assert gpu.spmv_csr_multi(A.handle, d_x, d_y, k, config=cfg).error_code == 0
            assert not gpu.csr_has_tiled_plan(A.handle), call
        # and a single-vector caller still promotes after its own four calls, not earlier
        x1, y1 = wl.vector_device(8, 2, n), gpu.CudaBuffer(n)
        for call in range(5):
            assert gpu.spmv_csr(A.handle, x1, y1, gpu.SpMVConfig(VECTOR), n).error_code == 0
            assert gpu.csr_has_tiled_plan(A.handle) == (call == 4), call
    finally:
        gpu.set_tiled_promotion(before)
    A.close()


def test_single_vector_merge_path_unchanged_by_multi_calls(gpu, shapes):
    M = shapes["long_row"]
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, M.cols).astype(np.float32)
    d_x, d_y = gpu.CudaBuffer(M.cols), gpu.CudaBuffer(M.rows)
    d_x.copyFromHost(x, M.cols)
    merge = gpu.SpMVConfig(MERGE)
    assert gpu.spmv_csr(M.A, d_x, d_y, merge, M.cols).error_code == 0
    first = d_y.copyToHost(M.rows).view(np.uint32).copy()
    for k in (8, 33, 1, 64):
        X = _x(rng, M.cols, k)
        _run(gpu, M, X, k, k, k, MERGE)
        assert gpu.spmv_csr(M.A, d_x, d_y, merge, M.cols).error_code == 0
        assert np.array_equal(d_y.copyToHost(M.rows).view(np.uint32), first), k


def test_changed_values_after_invalidate(gpu, oracle):
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 40, 3000)
    rp, ci, va = gpu.synth.stratified_csr(3, 0, lens, 2000)
    M = Host(gpu, 3000, 2000, rp, ci, va)
    k = 8
    X = _x(rng, M.cols, k)
    for kernel in (SCALAR, VECTOR, MERGE):
        _run(gpu, M, X, k, k, k, kernel)
    M.va = (M.va * np.float32(-1.5) + np.float32(0.25)).astype(np.float32)
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(M.A.contents.d_values), M.va.ctypes.data_as(ctypes.c_void_p),
                                       M.va.nbytes) == 0
    gpu.csr_invalidate_gpu_cache(M.A)
    want = _oracle_cols(oracle, M, X, k)
    for kernel in (SCALAR, VECTOR, MERGE):
        bits, _ = _run(gpu, M, X, k, k, k, kernel)
        _check(bits, want, k, kernel, M, X)
    M.close()


# --------------------------------------------------------------------------------------------- async
def test_async_on_a_side_stream_equals_the_synchronous_call(gpu, shapes):
    torch = pytest.importorskip("torch")
    M = shapes["long_row"]
    rng = np.random.default_rng(13)
    side = torch.cuda.Stream()
    for kernel in (SCALAR, VECTOR, MERGE):
        for k in (3, 8, 40):
            X = _x(rng, M.cols, k)
            sync_bits, _ = _run(gpu, M, X, k, k, k + 1, kernel)
            d_x = gpu.CudaBuffer(X.size)
            d_x.copyFromHost(X.reshape(-1), X.size)
            d_y = gpu.CudaBuffer(M.rows * (k + 1))
            d_y.copyFromHost(np.full(M.rows * (k + 1), SENTINEL, np.uint32).view(np.float32), M.rows * (k + 1))
            status = gpu.spmv_csr_multi_async(M.A, d_x, d_y, k, k, k + 1, gpu.SpMVConfig(kernel), M.cols,
                                              side.cuda_stream)
            assert status == 0
            side.synchronize()
            got = d_y.copyToHost(M.rows * (k + 1)).view(np.uint32).reshape(M.rows, k + 1)
            assert np.array_equal(got, sync_bits), (kernel, k)


# ------------------------------------------------------------------------------------ 64-bit offsets
SEED, TAG = 77, 5


def _unit_at(idx):
    return importlib.import_module("gpu-spmv_amd").synth.to_unit(
        importlib.import_module("gpu-spmv_amd").synth.draw(SEED, 3, TAG, np.asarray(idx, np.uint64)))


def test_x_offsets_past_2_to_the_31(gpu, oracle):
    num_cols, ldx, k, rows = (1 << 22) + 64, 512, 4, 64
    assert num_cols * ldx > 2**31
    rng = np.random.default_rng(21)
    lens = rng.integers(1, 6, rows)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = (num_cols - 64 + rng.integers(0, 64, rp[-1])).astype(np.int32)
    va = rng.uniform(-1, 1, rp[-1]).astype(np.float32)
    M = Host(gpu, rows, num_cols, rp, ci, va)
    used = (num_cols - 1) * ldx + k
    d_x = gpu.CudaBuffer(used)
    assert gpu.lib().spmv_c_gen_vector(SEED, TAG, used, d_x.get(), None) == 0
    want = []
    needed = np.unique(ci)
    for j in range(k):
        x = np.zeros(num_cols, np.float32)
        x[needed] = _unit_at(needed.astype(np.uint64) * ldx + j)
        want.append(oracle.spmv_csr(rp, ci, va, x))
    d_y = gpu.CudaBuffer(rows * k)
    for kernel in (SCALAR, VECTOR, MERGE):
        assert gpu.spmv_csr_multi(M.A, d_x, d_y, k, ldx, k, gpu.SpMVConfig(kernel), num_cols).error_code == 0
        Y = d_y.copyToHost(rows * k).reshape(rows, k)
        for j in range(k):
            if kernel == SCALAR:
                np.testing.assert_array_equal(Y[:, j], want[j])
            else:
                x = np.zeros(num_cols, np.float32)
                x[needed] = _unit_at(needed.astype(np.uint64) * ldx + j)
                assert reorder_err(rp, ci, va, x, want[j], Y[:, j]) <= TOL, (kernel, j)
    d_x.release()
    M.close()


def test_y_offsets_past_2_to_the_31(gpu, oracle):
    num_rows, ldy, k, cols, tail = (1 << 22) + 64, 512, 4, 1000, 64
    assert num_rows * ldy > 2**31
    rng = np.random.default_rng(22)
    lens = np.zeros(num_rows, np.int64)
    lens[-tail:] = rng.integers(1, 30, tail)
    lens[::100_003] = 3                                 # a few entries early on too
    rp, ci, va = gpu.synth.stratified_csr(6, 0, lens, cols)
    M = Host(gpu, num_rows, cols, rp, ci, va)
    X = _x(rng, cols, k)
    d_x = gpu.CudaBuffer(X.size)
    d_x.copyFromHost(X.reshape(-1), X.size)
    want = [oracle.spmv_csr(rp, ci, va, np.ascontiguousarray(X[:, j])) for j in range(k)]
    used = (num_rows - 1) * ldy + k
    d_y = gpu.CudaBuffer(used)
    first = (num_rows - tail) * ldy                     # the last `tail` rows, padding included (but past the end)
    span = used - first
    tail_ptr = ctypes.c_void_p(d_y.get() + 4 * first)
    for kernel in (SCALAR, VECTOR, MERGE):
        fill = np.full(span, SENTINEL, np.uint32)
        assert gpu.lib().spmv_c_memcpy_h2d(tail_ptr, fill.ctypes.data_as(ctypes.c_void_p), fill.nbytes) == 0
        assert gpu.spmv_csr_multi(M.A, d_x, d_y, k, k, ldy, gpu.SpMVConfig(kernel), cols).error_code == 0
        got = np.empty(span, np.uint32)
        assert gpu.lib().spmv_c_memcpy_d2h(got.ctypes.data_as(ctypes.c_void_p), tail_ptr, got.nbytes) == 0
        got = np.concatenate([got, np.full(ldy - k, SENTINEL, np.uint32)]).reshape(tail, ldy)
        assert np.all(got[:, k:] == SENTINEL), kernel
        Y = got[:, :k].view(np.float32)
        for j in range(k):
            w = want[j][-tail:]
            if kernel == SCALAR:
                np.testing.assert_array_equal(Y[:, j], w)
            else:
                sub_rp = (rp[-tail - 1:] - rp[-tail - 1]).astype(np.int64)
                sl = slice(int(rp[-tail - 1]), int(rp[-1]))
                assert reorder_err(sub_rp, ci[sl], va[sl], X[:, j], w, Y[:, j]) <= TOL, (kernel, j)
    d_y.release()
    M.close()


# ------------------------------------------------------------------------------------- C++ drop-in
def test_cpp_multi_smoke(gpu, tmp_path):
    """tests/cpp/multi_smoke.cpp through spmv/spmv.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "multi_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "multi_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
