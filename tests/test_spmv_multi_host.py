"""spmv_csr_multi on the host side (no GPU): the C ABI's argument checks that come before any device work, and
the multi-vector byte model (include/spmv/bandwidth.h)."""
import ctypes

import numpy as np
import pytest


def _matrix(spmv, rows=8, cols=6):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, (i * 5) % cols] = 1.5 + i
        dense[i, (i * 3 + 1) % cols] = -0.5
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


def test_c_abi_rejects_null_arguments_and_bad_k_without_a_device(spmv):
    lib = spmv.lib()
    E = spmv.SpMVError
    A = _matrix(spmv)
    # fake, never-dereferenced device addresses: every call below must return before touching them
    X, Y = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)
    out = spmv.SpMVResult()
    assert lib.spmv_c_spmv_csr_multi(None, X, 4, Y, 4, 4, None, -1, ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT
    assert lib.spmv_c_spmv_csr_multi(A, None, 4, Y, 4, 4, None, -1, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spmv_csr_multi(A, X, 4, None, 4, 4, None, -1, None) == E.INVALID_ARGUMENT
    for k in (0, -1, -100):
        assert lib.spmv_c_spmv_csr_multi(A, X, 4, Y, 4, k, None, -1, None) == E.INVALID_ARGUMENT
        assert lib.spmv_c_spmv_csr_multi_async(A, X, 4, Y, 4, k, None, -1, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spmv_csr_multi_async(None, X, 4, Y, 4, 4, None, -1, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spmv_csr_multi_async(A, None, 4, Y, 4, 4, None, -1, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_spmv_csr_multi_async(A, X, 4, None, 4, 4, None, -1, None) == E.INVALID_ARGUMENT
    # the later checks, still before any device work: vec_size, leading dimensions, missing device arrays
    assert lib.spmv_c_spmv_csr_multi(A, X, 4, Y, 4, 4, None, 7, None) == E.INVALID_DIMENSION
    assert lib.spmv_c_spmv_csr_multi(A, X, 3, Y, 4, 4, None, 6, None) == E.INVALID_DIMENSION
    assert lib.spmv_c_spmv_csr_multi(A, X, 4, Y, 3, 4, None, -1, None) == E.INVALID_DIMENSION
    assert lib.spmv_c_spmv_csr_multi(A, X, 4, Y, 4, 4, None, 6, None) == E.INVALID_FORMAT   # never copied to a GPU
    # zero rows: a successful no-op, whatever k says
    Z = spmv.csr_create(0, 5, 0)
    assert lib.spmv_c_spmv_csr_multi(Z, X, 4, Y, 4, 0, None, -1, None) == E.SUCCESS
    spmv.csr_destroy(Z)
    spmv.csr_destroy(A)


def test_python_wrapper_defaults_leading_dimensions_to_k(spmv):
    A = _matrix(spmv)
    assert spmv.spmv_csr_multi(A, 0x1000, 0x100000, 4, vec_size=7).error_code == spmv.SpMVError.INVALID_DIMENSION
    assert spmv.spmv_csr_multi(A, 0x1000, 0x100000, 4, ldx=2).error_code == spmv.SpMVError.INVALID_DIMENSION
    assert spmv.spmv_csr_multi(A, 0x1000, 0x100000, 4).error_code == spmv.SpMVError.INVALID_FORMAT
    spmv.csr_destroy(A)


def test_multi_byte_model_at_k_1_is_the_csr_model_bit_for_bit(spmv):
    A = _matrix(spmv, 37, 23)
    for t in (0.001, 0.37, 1.0, 12.5):
        one = spmv.compute_bandwidth_csr(A, t)
        multi = spmv.compute_bandwidth_csr_multi(A, 1, t)
        assert bytes(one) == bytes(multi), t
    spmv.csr_destroy(A)


def test_multi_byte_model_at_k_8_matches_the_formula(spmv):
    rows, cols = 37, 23
    A = _matrix(spmv, rows, cols)
    nnz = A.contents.nnz
    k, t = 8, 0.25
    m = spmv.compute_bandwidth_csr_multi(A, k, t)
    want = (nnz * 8 + (rows + 1) * 4 + k * cols * 4 + k * rows * 4) / 1e9 / (t / 1e3)
    assert m.achieved_bandwidth_gb_s == pytest.approx(want, rel=1e-6)
    assert 0 < m.theoretical_bandwidth_gb_s < 10000 and 0 <= m.efficiency <= 1
    z = spmv.compute_bandwidth_csr_multi(A, k, 0.0)
    assert (z.achieved_bandwidth_gb_s, z.theoretical_bandwidth_gb_s, z.efficiency) == (0.0, 0.0, 0.0)
    out = spmv.BandwidthMetrics()
    assert spmv.lib().spmv_c_compute_bandwidth_csr_multi(A, k, t, None) == spmv.SpMVError.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_compute_bandwidth_csr_multi(A, k, t, ctypes.byref(out)) == 0
    spmv.csr_destroy(A)
