"""csr_transpose_gpu / spmv_csr_transpose on the host side (no GPU): the argument checks of both calls that come
before any device work, in their documented order, and the C ABI / Python names."""
import ctypes

import numpy as np


def _matrix(spmv, rows=8, cols=6):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, (i * 5) % cols] = 1.5 + i
        dense[i, (i * 3 + 1) % cols] = -0.5
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


def test_names_exist_in_the_c_abi_and_the_python_mirror(spmv):
    lib = spmv.lib()
    for name in ("spmv_c_csr_transpose_gpu", "spmv_c_spmv_csr_transpose", "spmv_c_spmv_csr_transpose_async"):
        assert name in spmv.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    for name in ("csr_transpose_gpu", "spmv_csr_transpose", "spmv_csr_transpose_async"):
        assert callable(getattr(spmv, name))


def test_csr_transpose_gpu_checks_before_any_device_work(spmv):
    lib = spmv.lib()
    E = spmv.SpMVError
    A = _matrix(spmv)
    AT = spmv.csr_create(2, 3, 0)
    before = (AT.contents.num_rows, AT.contents.num_cols, AT.contents.nnz)
    # 1. null arguments
    assert lib.spmv_c_csr_transpose_gpu(None, A) == E.INVALID_ARGUMENT
    assert lib.spmv_c_csr_transpose_gpu(AT, None) == E.INVALID_ARGUMENT
    assert spmv.csr_transpose_gpu(None, None) == E.INVALID_ARGUMENT
    # 2. missing device arrays (A was never copied to a GPU)
    assert spmv.csr_transpose_gpu(AT, A) == E.INVALID_FORMAT
    H = spmv.csr_create(3, 4, 0)                       # rows > 0 and no device row pointers
    assert spmv.csr_transpose_gpu(AT, H) == E.INVALID_FORMAT
    spmv.csr_destroy(H)
    # a matrix with no rows cannot hold entries
    Z = spmv.csr_create(0, 4, 0)
    Z.contents.nnz = 3
    assert spmv.csr_transpose_gpu(AT, Z) == E.INVALID_FORMAT
    Z.contents.nnz = 0
    spmv.csr_destroy(Z)
    # AT untouched by every failure
    assert (AT.contents.num_rows, AT.contents.num_cols, AT.contents.nnz) == before
    assert not AT.contents.owns_device_memory
    spmv.csr_destroy(AT)
    spmv.csr_destroy(A)


def test_spmv_csr_transpose_checks_in_the_stated_order_without_a_device(spmv):
    lib = spmv.lib()
    E = spmv.SpMVError
    A = _matrix(spmv)                                  # 8 x 6, host only
    # fake, never-dereferenced device addresses: every call below must return before touching them
    X, Y = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000)
    out = spmv.SpMVResult()
    bad_block = spmv.SpMVConfig(0, 0)
    for sync in (True, False):
        def call(A=A, x=X, y=Y, cfg=None, vs=-1):
            if sync:
                return lib.spmv_c_spmv_csr_transpose(A, x, y, ctypes.byref(cfg) if cfg else None, vs,
                                                     ctypes.byref(out))
            return lib.spmv_c_spmv_csr_transpose_async(A, x, y, ctypes.byref(cfg) if cfg else None, vs, None)
        # 1. nulls, before everything else
        assert call(A=None, vs=99) == E.INVALID_ARGUMENT
        assert call(x=None, vs=99) == E.INVALID_ARGUMENT and call(y=None, vs=99) == E.INVALID_ARGUMENT
        # 2. zero columns: a successful no-op, whatever follows
        Z = spmv.csr_create(5, 0, 0)
        assert call(A=Z, vs=99, cfg=bad_block) == E.SUCCESS
        spmv.csr_destroy(Z)
        # 3. vec_size is checked against num_rows (x has num_rows entries), before the format check
        assert call(vs=6) == E.INVALID_DIMENSION
        assert call(vs=7, cfg=bad_block) == E.INVALID_DIMENSION
        # 4. missing device arrays, before the block size
        assert call(vs=8) == E.INVALID_FORMAT
        assert call(vs=-1, cfg=bad_block) == E.INVALID_FORMAT
    assert out.error_code == E.INVALID_FORMAT
    spmv.csr_destroy(A)


def test_python_wrappers_pass_their_arguments_through(spmv):
    E = spmv.SpMVError
    A = _matrix(spmv)
    assert spmv.spmv_csr_transpose(A, 0x1000, 0x100000, vec_size=6).error_code == E.INVALID_DIMENSION
    assert spmv.spmv_csr_transpose(A, 0x1000, 0x100000, spmv.SpMVConfig(1), 8).error_code == E.INVALID_FORMAT
    assert spmv.spmv_csr_transpose_async(A, 0x1000, 0x100000, None, 6) == E.INVALID_DIMENSION
    assert spmv.spmv_csr_transpose_async(A, 0, 0x100000) == E.INVALID_ARGUMENT
    spmv.csr_destroy(A)
