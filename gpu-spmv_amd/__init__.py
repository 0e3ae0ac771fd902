"""gpu-spmv_amd — Python host mirror of the MI355X-native SpMV library.

The product is ``lib/libspmv_amd.so`` (hand-written HIP kernels for gfx950 + the
C++ API in ``namespace spmv`` + the C ABI of ``include/spmv_c.h``).  This module
binds that C ABI with ctypes and mirrors the reference's interface
(LessUp/gpu-spmv ``include/spmv/*.h``): same function names, argument meaning
and error behaviour, so tests written against it read like the reference's own
(``tests/test_spmv.cu`` etc.).

There is no CPU fallback: importing works without a GPU (the library loads, the
host-side containers work), but every device entry point needs a HIP device and
the library itself must have been built (``python __graft_entry__.py`` or
``make -C gpu-spmv_amd``) — otherwise ``LibraryNotBuilt`` is raised.

The directory name carries a hyphen, so import it with
``importlib.import_module("gpu-spmv_amd")``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64
from ctypes import c_size_t, c_uint8, c_uint64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPMV_AMD_LIB") or os.path.join(_HERE, "lib", "libspmv_amd.so")   # SPMV_AMD_LIB: an A/B build of the same library (tools/)


class LibraryNotBuilt(ImportError):
    pass


class SpMVError:
    """reference include/spmv/common.h:13-23"""
    SUCCESS = 0
    INVALID_DIMENSION = -1
    CUDA_MALLOC = -2
    CUDA_MEMCPY = -3
    KERNEL_LAUNCH = -4
    INVALID_FORMAT = -5
    FILE_IO = -6
    OUT_OF_MEMORY = -7
    INVALID_ARGUMENT = -8


class CudaException(RuntimeError):
    """Raised by CudaBuffer on device allocation / copy failure (common.h:42-50)."""


# ---- struct mirrors (layouts asserted in csrc/capi.cpp) -----------------------------
class CSRMatrix(Structure):
    """reference include/spmv/csr_matrix.h:11-28"""
    _fields_ = [("num_rows", c_int32), ("num_cols", c_int32), ("nnz", c_int32),
                ("values", POINTER(c_float)), ("col_indices", POINTER(c_int32)),
                ("row_ptrs", POINTER(c_int32)),
                ("d_values", c_void_p), ("d_col_indices", c_void_p), ("d_row_ptrs", c_void_p),
                ("owns_host_memory", c_uint8), ("owns_device_memory", c_uint8)]


class ELLMatrix(Structure):
    """reference include/spmv/ell_matrix.h:12-28"""
    _fields_ = [("num_rows", c_int32), ("num_cols", c_int32), ("max_nnz_per_row", c_int32),
                ("values", POINTER(c_float)), ("col_indices", POINTER(c_int32)),
                ("d_values", c_void_p), ("d_col_indices", c_void_p),
                ("owns_host_memory", c_uint8), ("owns_device_memory", c_uint8)]


class CSRStats(Structure):
    """reference include/spmv/csr_matrix.h:64-69"""
    _fields_ = [("avg_nnz_per_row", c_float), ("max_nnz_per_row", c_int32),
                ("min_nnz_per_row", c_int32), ("skewness", c_float)]


class SpMVConfig(Structure):
    """reference include/spmv/spmv.h:11-24 (defaults SCALAR_CSR / 256 / False)"""
    SCALAR_CSR, VECTOR_CSR, MERGE_PATH, ELL_KERNEL = 0, 1, 2, 3
    _fields_ = [("kernel_type", c_int32), ("block_size", c_int32), ("use_texture", c_uint8)]

    def __init__(self, kernel_type=0, block_size=256, use_texture=False):
        super().__init__(kernel_type, block_size, 1 if use_texture else 0)


class SpMVResult(Structure):
    """reference include/spmv/spmv.h:27-36"""
    _fields_ = [("y", c_void_p), ("elapsed_ms", c_float), ("gflops", c_float),
                ("bandwidth_gb_s", c_float), ("error_code", c_int32)]


class BandwidthMetrics(Structure):
    """reference include/spmv/bandwidth.h:10-18"""
    _fields_ = [("theoretical_bandwidth_gb_s", c_float), ("achieved_bandwidth_gb_s", c_float),
                ("efficiency", c_float)]


class PageRankConfig(Structure):
    """reference include/spmv/pagerank.h:9-15 (defaults 0.85 / 1e-6 / 100)"""
    _fields_ = [("damping_factor", c_float), ("tolerance", c_float), ("max_iterations", c_int32)]

    def __init__(self, damping_factor=0.85, tolerance=1e-6, max_iterations=100):
        super().__init__(damping_factor, tolerance, max_iterations)


class _PageRankResultC(Structure):
    _fields_ = [("ranks", POINTER(c_float)), ("iterations", c_int32), ("final_residual", c_float),
                ("converged", c_uint8)]


class TopKNode(Structure):
    """reference include/spmv/pagerank.h:38-41"""
    _fields_ = [("node_id", c_int32), ("rank", c_float)]


class PrStatus(Structure):
    _fields_ = [("dangling_sum", c_float), ("final_residual", c_float), ("iterations", c_int32),
                ("converged", c_int32), ("done", c_int32), ("reserved", c_int32)]


class CGConfig(Structure):
    """include/spmv/cg.h CGConfig (16 bytes): preconditioner 0 NONE / 1 JACOBI; engine -1 auto, 0 direct, 1 tiled"""
    _fields_ = [("tolerance", c_float), ("max_iterations", c_int32), ("preconditioner", c_int32),
                ("engine", c_int32)]
    NONE, JACOBI = 0, 1

    def __init__(self, tolerance=1e-6, max_iterations=1000, preconditioner=1, engine=-1):
        super().__init__(tolerance, max_iterations, preconditioner, engine)


class CGResult(Structure):
    """include/spmv/cg.h CGResult (24 bytes)"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("relative_residual", c_float),
                ("converged", c_int32), ("breakdown", c_int32), ("elapsed_ms", c_float)]


class PersonalizedResult(Structure):
    """include/spmv/pagerank.h PersonalizedResult (20 bytes), one per teleport vector"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("final_residual", c_float),
                ("converged", c_int32), ("elapsed_ms", c_float)]


class BiCGStabConfig(Structure):
    """include/spmv/bicgstab.h BiCGStabConfig (16 bytes): the fields, defaults and meanings of CGConfig"""
    _fields_ = [("tolerance", c_float), ("max_iterations", c_int32), ("preconditioner", c_int32),
                ("engine", c_int32)]
    NONE, JACOBI = 0, 1

    def __init__(self, tolerance=1e-6, max_iterations=1000, preconditioner=1, engine=-1):
        super().__init__(tolerance, max_iterations, preconditioner, engine)


# BiCGStabResult.breakdown codes (include/spmv/bicgstab.h BiCGStabResult::Breakdown)
BICGSTAB_NO_BREAKDOWN, BICGSTAB_RHO, BICGSTAB_ALPHA, BICGSTAB_OMEGA = 0, 1, 2, 3


class BiCGStabResult(Structure):
    """include/spmv/bicgstab.h BiCGStabResult (24 bytes); breakdown is one of NONE, RHO, ALPHA, OMEGA"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("relative_residual", c_float),
                ("converged", c_int32), ("breakdown", c_int32), ("elapsed_ms", c_float)]
    NONE, RHO, ALPHA, OMEGA = BICGSTAB_NO_BREAKDOWN, BICGSTAB_RHO, BICGSTAB_ALPHA, BICGSTAB_OMEGA


class GMRESConfig(Structure):
    """include/spmv/gmres.h GMRESConfig (20 bytes): restart 1..64; the other fields as CGConfig"""
    _fields_ = [("tolerance", c_float), ("max_iterations", c_int32), ("restart", c_int32),
                ("preconditioner", c_int32), ("engine", c_int32)]
    NONE, JACOBI = 0, 1

    def __init__(self, tolerance=1e-6, max_iterations=1000, restart=30, preconditioner=1, engine=-1):
        super().__init__(tolerance, max_iterations, restart, preconditioner, engine)


# GMRESResult.breakdown codes (include/spmv/gmres.h GMRESResult::Breakdown)
GMRES_NO_BREAKDOWN, GMRES_SINGULAR, GMRES_NOT_FINITE = 0, 1, 2


class GMRESResult(Structure):
    """include/spmv/gmres.h GMRESResult (28 bytes); breakdown is one of NONE, SINGULAR, NOT_FINITE"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("restarts", c_int32),
                ("relative_residual", c_float), ("converged", c_int32), ("breakdown", c_int32),
                ("elapsed_ms", c_float)]
    NONE, SINGULAR, NOT_FINITE = GMRES_NO_BREAKDOWN, GMRES_SINGULAR, GMRES_NOT_FINITE


class MinresConfig(Structure):
    """include/spmv/minres.h MinresConfig (20 bytes): solves (A - shift I) x = b; preconditioner 0 NONE / 1 JACOBI
    (M = |diag(A - shift I)|); the other fields as CGConfig"""
    _fields_ = [("tolerance", c_float), ("max_iterations", c_int32), ("preconditioner", c_int32),
                ("engine", c_int32), ("shift", c_float)]
    NONE, JACOBI = 0, 1

    def __init__(self, tolerance=1e-6, max_iterations=1000, preconditioner=1, engine=-1, shift=0.0):
        super().__init__(tolerance, max_iterations, preconditioner, engine, shift)


# MinresResult.breakdown codes (include/spmv/minres.h MinresResult::Breakdown)
MINRES_NO_BREAKDOWN, MINRES_PRECONDITIONER, MINRES_NOT_FINITE, MINRES_SINGULAR = 0, 1, 2, 3


class MinresResult(Structure):
    """include/spmv/minres.h MinresResult (28 bytes); relative_residual is the recurrence's (M^-1-norm),
    true_relative_residual the recomputed 2-norm one; breakdown is one of NONE, PRECONDITIONER, NOT_FINITE, SINGULAR"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("relative_residual", c_float),
                ("true_relative_residual", c_float), ("converged", c_int32), ("breakdown", c_int32),
                ("elapsed_ms", c_float)]
    NONE, PRECONDITIONER, NOT_FINITE, SINGULAR = (MINRES_NO_BREAKDOWN, MINRES_PRECONDITIONER, MINRES_NOT_FINITE,
                                                  MINRES_SINGULAR)


class EigsConfig(Structure):
    """include/spmv/eigs.h EigsConfig (24 bytes): num_values 1..32; which 0 LARGEST / 1 SMALLEST (algebraic); basis 0
    (= min(max(2 num_values, 20), 64)) or in (num_values, 64]; engine as CGConfig"""
    _fields_ = [("num_values", c_int32), ("which", c_int32), ("basis", c_int32), ("tolerance", c_float),
                ("max_iterations", c_int32), ("engine", c_int32)]
    LARGEST, SMALLEST = 0, 1

    def __init__(self, num_values=1, which=0, basis=0, tolerance=1e-5, max_iterations=1000, engine=-1):
        super().__init__(num_values, which, basis, tolerance, max_iterations, engine)


# EigsResult.breakdown codes (include/spmv/eigs.h EigsResult::Breakdown)
EIGS_NO_BREAKDOWN, EIGS_INVARIANT_SUBSPACE, EIGS_NOT_FINITE = 0, 1, 2
# the default start vector of eigs_sym: synth.vector(EIGS_START_SEED, EIGS_START_TAG, n)
EIGS_START_SEED, EIGS_START_TAG = 0x45494753, 0


class EigsResult(Structure):
    """include/spmv/eigs.h EigsResult (28 bytes); converged counts the returned pairs whose recomputed residual passes;
    breakdown is one of NONE, INVARIANT_SUBSPACE, NOT_FINITE"""
    _fields_ = [("error_code", c_int32), ("iterations", c_int32), ("restarts", c_int32), ("converged", c_int32),
                ("breakdown", c_int32), ("max_residual", c_float), ("elapsed_ms", c_float)]
    NONE, INVARIANT_SUBSPACE, NOT_FINITE = EIGS_NO_BREAKDOWN, EIGS_INVARIANT_SUBSPACE, EIGS_NOT_FINITE


class SpTRSVConfig(Structure):
    """include/spmv/sptrsv.h SpTRSVConfig (16 bytes): uplo 0 LOWER / 1 UPPER; diag 0 NON_UNIT / 1 UNIT; ordered 1 = one
    lane per row in the CPU's summation order"""
    _fields_ = [("uplo", c_int32), ("diag", c_int32), ("ordered", c_int32), ("reserved", c_int32)]
    LOWER, UPPER = 0, 1
    NON_UNIT, UNIT = 0, 1

    def __init__(self, uplo=0, diag=0, ordered=0, reserved=0):
        super().__init__(uplo, diag, ordered, reserved)


class SpTRSVResult(Structure):
    """include/spmv/sptrsv.h SpTRSVResult (24 bytes)"""
    _fields_ = [("error_code", c_int32), ("num_levels", c_int32), ("launches", c_int32),
                ("lanes_per_row", c_int32), ("analysis_ms", c_float), ("elapsed_ms", c_float)]


class SpTRSVScheduleInfo(Structure):
    """include/spmv/sptrsv.h SpTRSVScheduleInfo (32 bytes): what a cached level schedule holds besides its arrays"""
    _fields_ = [("num_levels", c_int32), ("launches", c_int32), ("first_missing_diagonal", c_int32),
                ("first_unsorted_row", c_int32), ("one_sided_row", c_int32), ("built_on_device", c_int32),
                ("triangle_nnz", c_int64)]


class ILU0Result(Structure):
    """include/spmv/ilu0.h ILU0Result (28 bytes); zero_pivot is the lowest row with a zero or non-finite u_ii, or -1"""
    _fields_ = [("error_code", c_int32), ("num_levels", c_int32), ("launches", c_int32),
                ("lanes_per_row", c_int32), ("zero_pivot", c_int32), ("analysis_ms", c_float),
                ("elapsed_ms", c_float)]


class IC0Result(Structure):
    """include/spmv/ic0.h IC0Result (28 bytes); bad_pivot is the lowest row whose l_ii is not > 0 or not finite, or -1"""
    _fields_ = [("error_code", c_int32), ("num_levels", c_int32), ("launches", c_int32),
                ("lanes_per_row", c_int32), ("bad_pivot", c_int32), ("analysis_ms", c_float),
                ("elapsed_ms", c_float)]


class ColorConfig(Structure):
    """include/spmv/reorder.h ColorConfig (16 bytes): the seed of the vertex priorities; symmetric_pattern 1 = only A's
    rows are walked; lanes_per_row 0 = from the mean degree, else 1, 2, 4, ... 64"""
    _fields_ = [("seed", ctypes.c_uint32), ("symmetric_pattern", c_int32), ("lanes_per_row", c_int32),
                ("reserved", c_int32)]

    def __init__(self, seed=0, symmetric_pattern=0, lanes_per_row=0, reserved=0):
        super().__init__(seed, symmetric_pattern, lanes_per_row, reserved)


class ColorResult(Structure):
    """include/spmv/reorder.h ColorResult (20 bytes)"""
    _fields_ = [("error_code", c_int32), ("num_colors", c_int32), ("rounds", c_int32), ("launches", c_int32),
                ("elapsed_ms", c_float)]


class RcmConfig(Structure):
    """include/spmv/reorder.h RcmConfig (16 bytes): symmetric_pattern 1 = only A's rows are walked; peripheral 1 = a
    pseudo-peripheral start per component; lanes_per_row 0 = from the mean degree, else 1, 2, 4, ... 64"""
    _fields_ = [("symmetric_pattern", c_int32), ("peripheral", c_int32), ("lanes_per_row", c_int32),
                ("reserved", c_int32)]

    def __init__(self, symmetric_pattern=0, peripheral=1, lanes_per_row=0, reserved=0):
        super().__init__(symmetric_pattern, peripheral, lanes_per_row, reserved)


class RcmResult(Structure):
    """include/spmv/reorder.h RcmResult (24 bytes)"""
    _fields_ = [("error_code", c_int32), ("components", c_int32), ("levels", c_int32), ("sweeps", c_int32),
                ("launches", c_int32), ("elapsed_ms", c_float)]


class CsrBand(Structure):
    """include/spmv/reorder.h CsrBand (16 bytes): max(i - j), max(j - i) over the stored entries and the profile"""
    _fields_ = [("lower", c_int32), ("upper", c_int32), ("profile", ctypes.c_int64)]


class CooConfig(Structure):
    """include/spmv/assemble.h CooConfig (8 bytes): duplicates COO_SUM (0) = equal (row, column) pairs are summed in
    source order, COO_KEEP (1) = every triplet becomes an entry"""
    _fields_ = [("duplicates", c_int32), ("reserved", c_int32)]
    COO_SUM, COO_KEEP = 0, 1

    def __init__(self, duplicates=0, reserved=0):
        super().__init__(duplicates, reserved)


class CooResult(Structure):
    """include/spmv/assemble.h CooResult (28 bytes); tile_entries is the number of entries one workgroup sorts per
    radix pass"""
    _fields_ = [("error_code", c_int32), ("nnz_out", c_int32), ("combined", c_int32), ("passes", c_int32),
                ("tile_entries", c_int32), ("launches", c_int32), ("elapsed_ms", c_float)]


class CsrAddResult(Structure):
    """include/spmv/csr_ops.h CsrAddResult (32 bytes); common counts the columns found in both matrices, launches the
    kernel launches of the call"""
    _fields_ = [("error_code", c_int32), ("nnz", c_int32), ("common", c_int32), ("max_row_nnz", c_int32),
                ("lanes", c_int32), ("launches", c_int32), ("symbolic_ms", c_float), ("numeric_ms", c_float)]


class BSRMatrix(Structure):
    """include/spmv/bsr_matrix.h BSRMatrix (80 bytes): square block_dim x block_dim blocks, row-major inside a block"""
    _fields_ = [("num_rows", c_int32), ("num_cols", c_int32), ("block_dim", c_int32), ("num_block_rows", c_int32),
                ("num_block_cols", c_int32), ("num_blocks", c_int32),
                ("values", POINTER(c_float)), ("block_cols", POINTER(c_int32)), ("block_row_ptrs", POINTER(c_int32)),
                ("d_values", c_void_p), ("d_block_cols", c_void_p), ("d_block_row_ptrs", c_void_p),
                ("owns_host_memory", c_uint8), ("owns_device_memory", c_uint8)]


class BsrBuildResult(Structure):
    """include/spmv/bsr.h BsrBuildResult (32 bytes); fill = nnz / positions of the blocks that lie inside the matrix"""
    _fields_ = [("error_code", c_int32), ("num_blocks", c_int32), ("fill", c_float), ("max_block_row", c_int32),
                ("lanes", c_int32), ("launches", c_int32), ("symbolic_ms", c_float), ("numeric_ms", c_float)]


class FSAIResult(Structure):
    """include/spmv/fsai.h FSAIResult (32 bytes); bad_row is the lowest row whose g_ii is not > 0 or not finite, long_row
    the lowest row with more than 64 pattern entries, -1 when there is none"""
    _fields_ = [("error_code", c_int32), ("nnz", c_int32), ("max_row", c_int32), ("row_class", c_int32),
                ("lanes_per_row", c_int32), ("bad_row", c_int32), ("long_row", c_int32), ("elapsed_ms", c_float)]


class SpGEMMResult(Structure):
    """include/spmv/spgemm.h SpGEMMResult (104 bytes); symbolic_rows / numeric_rows count the rows per accumulator
    class of each pass, [0] the rows without products"""
    _fields_ = [("error_code", c_int32), ("nnz", c_int32), ("products", c_int64), ("max_row_products", c_int32),
                ("max_row_nnz", c_int32), ("symbolic_rows", c_int32 * 8), ("numeric_rows", c_int32 * 8),
                ("lanes", c_int32), ("symbolic_ms", c_float), ("numeric_ms", c_float)]


class AMGConfig(Structure):
    """include/spmv/amg.h AMGConfig (28 bytes), with its defaults"""
    _fields_ = [("max_levels", c_int32), ("coarse_rows", c_int32), ("strength", c_float), ("pre_sweeps", c_int32),
                ("post_sweeps", c_int32), ("jacobi_weight", c_float), ("coarse_sweeps", c_int32)]

    def __init__(self, max_levels=10, coarse_rows=64, strength=0.08, pre_sweeps=1, post_sweeps=1,
                 jacobi_weight=2.0 / 3.0, coarse_sweeps=4):
        super().__init__(max_levels, coarse_rows, strength, pre_sweeps, post_sweeps, jacobi_weight, coarse_sweeps)


class AMGSmoothing(Structure):
    """include/spmv/amg.h AMGSmoothing (8 bytes), with its defaults"""
    _fields_ = [("prolongator_weight", c_float), ("strength_decay", c_float)]

    def __init__(self, prolongator_weight=2.0 / 3.0, strength_decay=0.5):
        super().__init__(prolongator_weight, strength_decay)


class AMGResult(Structure):
    """include/spmv/amg.h AMGResult (48 bytes); bad_level / bad_row name the row a diagonal or pivot check failed at"""
    _fields_ = [("error_code", c_int32), ("levels", c_int32), ("coarse_solver", c_int32), ("bad_row", c_int32),
                ("bad_level", c_int32), ("grid_complexity", c_double), ("operator_complexity", c_double),
                ("setup_ms", c_float)]


class PageRankResult:
    """reference include/spmv/pagerank.h:18-25; `ranks` is a numpy copy (the C buffer is freed)."""

    def __init__(self, ranks, iterations, final_residual, converged):
        self.ranks = ranks
        self.iterations = iterations
        self.final_residual = final_residual
        self.converged = converged


# ---- library loading -----------------------------------------------------------------
_lib = None

_SIGNATURES = {
    # name: (restype, argtypes)
    "spmv_c_error_string": (c_char_p, [c_int]),
    "spmv_c_version": (c_char_p, []),
    "spmv_c_device_count": (c_int, []),
    "spmv_c_device_name": (c_int, [c_char_p, c_size_t]),
    "spmv_c_set_device": (c_int, [c_int]),
    "spmv_c_enable_peer_access": (c_int, [c_int]),
    "spmv_c_set_stream": (None, [c_void_p]),
    "spmv_c_device_malloc": (c_int, [POINTER(c_void_p), c_size_t]),
    "spmv_c_device_free": (c_int, [c_void_p]),
    "spmv_c_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t]),
    "spmv_c_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t]),
    "spmv_c_device_synchronize": (c_int, []),
    "spmv_c_ipc_get_handle": (c_int, [c_void_p, c_char_p]),
    "spmv_c_ipc_open_handle": (c_int, [c_char_p, POINTER(c_void_p)]),
    "spmv_c_ipc_close": (c_int, [c_void_p]),
    "spmv_c_csr_create": (POINTER(CSRMatrix), [c_int, c_int, c_int]),
    "spmv_c_csr_destroy": (None, [POINTER(CSRMatrix)]),
    "spmv_c_csr_from_dense": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_int]),
    "spmv_c_csr_to_dense": (c_int, [POINTER(CSRMatrix), c_void_p]),
    "spmv_c_csr_get_element": (c_float, [POINTER(CSRMatrix), c_int, c_int]),
    "spmv_c_csr_to_gpu": (c_int, [POINTER(CSRMatrix)]),
    "spmv_c_csr_from_gpu": (c_int, [POINTER(CSRMatrix)]),
    "spmv_c_csr_free_gpu": (None, [POINTER(CSRMatrix)]),
    "spmv_c_csr_invalidate_gpu_cache": (None, [POINTER(CSRMatrix)]),
    "spmv_c_csr_serialize": (c_int, [POINTER(CSRMatrix), c_char_p]),
    "spmv_c_csr_deserialize": (c_int, [POINTER(CSRMatrix), c_char_p]),
    "spmv_c_csr_compute_stats": (c_int, [POINTER(CSRMatrix), POINTER(CSRStats)]),
    "spmv_c_csr_wrap_device": (POINTER(CSRMatrix), [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_ell_create": (POINTER(ELLMatrix), [c_int, c_int, c_int]),
    "spmv_c_ell_destroy": (None, [POINTER(ELLMatrix)]),
    "spmv_c_ell_from_dense": (c_int, [POINTER(ELLMatrix), c_void_p, c_int, c_int]),
    "spmv_c_ell_from_csr": (c_int, [POINTER(ELLMatrix), POINTER(CSRMatrix)]),
    "spmv_c_ell_from_csr_gpu": (c_int, [POINTER(ELLMatrix), POINTER(CSRMatrix)]),
    "spmv_c_csr_transpose_gpu": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix)]),
    "spmv_c_ell_to_dense": (c_int, [POINTER(ELLMatrix), c_void_p]),
    "spmv_c_ell_get_element": (c_float, [POINTER(ELLMatrix), c_int, c_int]),
    "spmv_c_ell_to_gpu": (c_int, [POINTER(ELLMatrix)]),
    "spmv_c_ell_from_gpu": (c_int, [POINTER(ELLMatrix)]),
    "spmv_c_ell_free_gpu": (None, [POINTER(ELLMatrix)]),
    "spmv_c_ell_invalidate_gpu_cache": (None, [POINTER(ELLMatrix)]),
    "spmv_c_ell_serialize": (c_int, [POINTER(ELLMatrix), c_char_p]),
    "spmv_c_ell_deserialize": (c_int, [POINTER(ELLMatrix), c_char_p]),
    "spmv_c_ell_index": (c_int, [c_int, c_int, c_int]),
    "spmv_c_ell_wrap_device": (POINTER(ELLMatrix), [c_int, c_int, c_int, c_void_p, c_void_p]),
    "spmv_c_cpu_csr": (None, [POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_cpu_ell": (None, [POINTER(ELLMatrix), c_void_p, c_void_p]),
    "spmv_c_spmv_csr": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                POINTER(SpMVResult)]),
    "spmv_c_spmv_ell": (c_int, [POINTER(ELLMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                POINTER(SpMVResult)]),
    "spmv_c_auto_config": (c_int, [POINTER(CSRMatrix), POINTER(SpMVConfig)]),
    "spmv_c_validate_dimensions": (c_int, [c_int, c_int]),
    "spmv_c_csr_has_tiled_plan": (c_int, [POINTER(CSRMatrix)]),
    "spmv_c_set_tiled_promotion": (None, [c_int]),
    "spmv_c_get_tiled_promotion": (c_int, []),
    "spmv_c_tiled_shape": (c_int, [c_int64, c_int64, c_int64, POINTER(c_int32), POINTER(c_int32)]),
    "spmv_c_csr_tiled_info": (c_int, [POINTER(CSRMatrix), POINTER(c_int64)]),
    "spmv_c_csr_tiled_stats": (c_int, [POINTER(CSRMatrix), POINTER(c_double)]),
    "spmv_c_csr_tiled_checksum": (c_int, [POINTER(CSRMatrix), POINTER(c_uint64)]),
    "spmv_c_csr_tiled_folded": (c_int, [POINTER(CSRMatrix)]),
    "spmv_c_csr_tiled_items": (c_int, [POINTER(CSRMatrix)]),
    "spmv_c_csr_tiled_col_bytes": (c_int64, [POINTER(CSRMatrix)]),
    "spmv_c_ell_tiled_info": (c_int, [POINTER(ELLMatrix), POINTER(c_int64)]),
    "spmv_c_csr_transpose_tiled_info": (c_int, [POINTER(CSRMatrix), POINTER(c_int64)]),
    "spmv_c_spmv_csr_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                      c_void_p]),
    "spmv_c_spmv_ell_async": (c_int, [POINTER(ELLMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                      c_void_p]),
    "spmv_c_spmv_csr_multi": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                      POINTER(SpMVConfig), c_int, POINTER(SpMVResult)]),
    "spmv_c_spmv_csr_multi_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                            POINTER(SpMVConfig), c_int, c_void_p]),
    "spmv_c_spmv_csr_transpose": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                          POINTER(SpMVResult)]),
    "spmv_c_spmv_csr_transpose_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                                c_void_p]),
    "spmv_c_cg_solve": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(CGConfig), POINTER(CGResult)]),
    "spmv_c_bicgstab_solve": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(BiCGStabConfig),
                                      POINTER(BiCGStabResult)]),
    "spmv_c_bicgstab_solve_lu": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p,
                                         POINTER(BiCGStabConfig), POINTER(BiCGStabResult)]),
    "spmv_c_gmres_solve": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(GMRESConfig),
                                   POINTER(GMRESResult)]),
    "spmv_c_gmres_solve_lu": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p,
                                      POINTER(GMRESConfig), POINTER(GMRESResult)]),
    "spmv_c_minres_solve": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(MinresConfig),
                                    POINTER(MinresResult)]),
    "spmv_c_minres_solve_ic": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p,
                                       POINTER(MinresConfig), POINTER(MinresResult)]),
    "spmv_c_eigs_sym": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                POINTER(EigsConfig), POINTER(EigsResult)]),
    "spmv_c_sym_eig_small": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "spmv_c_ilu0_csr": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(ILU0Result)]),
    "spmv_c_ilu0_csr_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_ilu0_cpu_csr": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(c_int32)]),
    "spmv_c_cg_solve_multi": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int, POINTER(CGConfig),
                                      POINTER(CGResult)]),
    "spmv_c_cg_solve_ic": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(CGConfig),
                                   POINTER(CGResult)]),
    "spmv_c_ic0_csr": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(IC0Result)]),
    "spmv_c_ic0_csr_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_ic0_cpu_csr": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(c_int32)]),
    "spmv_c_fsai_csr": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(FSAIResult)]),
    "spmv_c_fsai_csr_numeric": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(FSAIResult)]),
    "spmv_c_fsai_cpu_csr": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(c_int32)]),
    "spmv_c_cg_solve_fsai": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p,
                                     POINTER(CGConfig), POINTER(CGResult)]),
    "spmv_c_spgemm_csr": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(SpGEMMResult)]),
    "spmv_c_spgemm_csr_numeric": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix),
                                          POINTER(SpGEMMResult)]),
    "spmv_c_spgemm_cpu_csr": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), POINTER(CSRMatrix)]),
    "spmv_c_spgemm_class_capacity": (c_int, [c_int]),
    "spmv_c_amg_setup": (c_int, [POINTER(c_void_p), POINTER(CSRMatrix), POINTER(AMGConfig), c_int,
                                 POINTER(c_void_p), POINTER(AMGResult)]),
    "spmv_c_amg_update": (c_int, [c_void_p, POINTER(CSRMatrix), POINTER(AMGResult)]),
    "spmv_c_amg_destroy": (None, [c_void_p]),
    "spmv_c_amg_num_levels": (c_int, [c_void_p]),
    "spmv_c_amg_level": (c_int, [c_void_p, c_int, POINTER(CSRMatrix), POINTER(c_void_p), POINTER(c_int32)]),
    "spmv_c_amg_apply": (c_int, [c_void_p, c_void_p, c_void_p]),
    "spmv_c_amg_aggregate_cpu_csr": (c_int, [POINTER(CSRMatrix), c_float, c_void_p, POINTER(c_int32)]),
    "spmv_c_amg_aggregate_mis2_cpu_csr": (c_int, [POINTER(CSRMatrix), c_float, ctypes.c_uint32, c_void_p, POINTER(c_int32),
                                                  POINTER(c_int32)]),
    "spmv_c_amg_aggregate_mis2_gpu": (c_int, [POINTER(CSRMatrix), c_float, ctypes.c_uint32, c_void_p, POINTER(c_int32),
                                              POINTER(c_int32)]),
    "spmv_c_amg_setup_device": (c_int, [POINTER(c_void_p), POINTER(CSRMatrix), POINTER(AMGConfig), ctypes.c_uint32,
                                        POINTER(AMGResult)]),
    "spmv_c_amg_setup_rounds": (c_int, [c_void_p, c_int]),
    "spmv_c_amg_setup_smoothed": (c_int, [POINTER(c_void_p), POINTER(CSRMatrix), POINTER(AMGConfig),
                                          POINTER(AMGSmoothing), c_int, POINTER(c_void_p), POINTER(AMGResult)]),
    "spmv_c_amg_setup_smoothed_device": (c_int, [POINTER(c_void_p), POINTER(CSRMatrix), POINTER(AMGConfig),
                                                 POINTER(AMGSmoothing), ctypes.c_uint32, POINTER(AMGResult)]),
    "spmv_c_amg_is_smoothed": (c_int, [c_void_p]),
    "spmv_c_amg_level_transfer": (c_int, [c_void_p, c_int, POINTER(CSRMatrix), POINTER(CSRMatrix)]),
    "spmv_c_amg_prolongator_cpu_csr": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_int, c_float]),
    "spmv_c_amg_restrict": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_amg_prolong": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    "spmv_c_cg_solve_amg": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, c_void_p, POINTER(CGConfig),
                                    POINTER(CGResult)]),
    "spmv_c_sptrsv_csr": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig),
                                  POINTER(SpTRSVResult)]),
    "spmv_c_sptrsv_csr_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig), c_void_p]),
    "spmv_c_sptrsv_analyze": (c_int, [POINTER(CSRMatrix), c_int, POINTER(SpTRSVResult)]),
    "spmv_c_sptrsv_analyze_device": (c_int, [POINTER(CSRMatrix), c_int, POINTER(SpTRSVResult)]),
    "spmv_c_sptrsv_schedule_get": (c_int, [POINTER(CSRMatrix), c_int, c_void_p, c_void_p,
                                           POINTER(SpTRSVScheduleInfo)]),
    "spmv_c_sptrsv_cpu_csr": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig)]),
    "spmv_c_sptrsv_csr_multi": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                        POINTER(SpTRSVConfig), POINTER(SpTRSVResult)]),
    "spmv_c_sptrsv_csr_multi_async": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                              POINTER(SpTRSVConfig), c_void_p]),
    "spmv_c_sptrsv_cpu_csr_multi": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                            POINTER(SpTRSVConfig)]),
    "spmv_c_cg_solve_multi_ic": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int,
                                         c_int, POINTER(CGConfig), POINTER(CGResult)]),
    "spmv_c_sptrsv_levels": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int32),
                                     POINTER(c_int32)]),
    "spmv_c_csr_color": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(ColorConfig), POINTER(ColorResult)]),
    "spmv_c_csr_color_cpu": (c_int, [POINTER(CSRMatrix), c_void_p, POINTER(c_int32), POINTER(c_int32),
                                     POINTER(ColorConfig)]),
    "spmv_c_color_ordering": (c_int, [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_csr_permute_gpu": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_csr_permute_cpu": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_permute_gather": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int]),
    "spmv_c_permute_gather_async": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    "spmv_c_multicolor_reorder": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p,
                                          POINTER(ColorConfig), POINTER(ColorResult)]),
    "spmv_c_csr_rcm": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(RcmConfig), POINTER(RcmResult)]),
    "spmv_c_csr_rcm_cpu": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(c_int32), POINTER(c_int32),
                                   POINTER(RcmConfig)]),
    "spmv_c_rcm_reorder": (c_int, [POINTER(CSRMatrix), POINTER(CSRMatrix), c_void_p, c_void_p, POINTER(RcmConfig),
                                   POINTER(RcmResult)]),
    "spmv_c_csr_band_gpu": (c_int, [POINTER(CSRMatrix), POINTER(CsrBand)]),
    "spmv_c_csr_band_cpu": (c_int, [POINTER(CSRMatrix), POINTER(CsrBand)]),
    "spmv_c_csr_from_coo_cpu": (c_int, [POINTER(CSRMatrix), c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        POINTER(CooConfig)]),
    "spmv_c_csr_from_coo_gpu": (c_int, [POINTER(CSRMatrix), c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        POINTER(CooConfig), POINTER(c_void_p), POINTER(CooResult)]),
    "spmv_c_csr_coo_refill": (c_int, [c_void_p, POINTER(CSRMatrix), c_void_p]),
    "spmv_c_csr_coo_refill_async": (c_int, [c_void_p, POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_coo_plan_destroy": (None, [c_void_p]),
    "spmv_c_coo_plan_info": (c_int, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                     POINTER(c_int32), POINTER(c_int32)]),
    "spmv_c_csr_row_indices_gpu": (c_int, [POINTER(CSRMatrix), c_void_p]),
    "spmv_c_csr_add": (c_int, [POINTER(CSRMatrix), c_float, POINTER(CSRMatrix), c_float, POINTER(CSRMatrix),
                               POINTER(CsrAddResult)]),
    "spmv_c_csr_add_numeric": (c_int, [POINTER(CSRMatrix), c_float, POINTER(CSRMatrix), c_float, POINTER(CSRMatrix),
                                       POINTER(CsrAddResult)]),
    "spmv_c_csr_add_cpu": (c_int, [POINTER(CSRMatrix), c_float, POINTER(CSRMatrix), c_float, POINTER(CSRMatrix)]),
    "spmv_c_bsr_create": (POINTER(BSRMatrix), [c_int, c_int, c_int, c_int]),
    "spmv_c_bsr_destroy": (None, [POINTER(BSRMatrix)]),
    "spmv_c_bsr_to_gpu": (c_int, [POINTER(BSRMatrix)]),
    "spmv_c_bsr_from_gpu": (c_int, [POINTER(BSRMatrix)]),
    "spmv_c_bsr_free_gpu": (None, [POINTER(BSRMatrix)]),
    "spmv_c_bsr_invalidate_gpu_cache": (None, [POINTER(BSRMatrix)]),
    "spmv_c_bsr_wrap_device": (POINTER(BSRMatrix), [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_bsr_from_csr_cpu": (c_int, [POINTER(BSRMatrix), POINTER(CSRMatrix), c_int]),
    "spmv_c_bsr_from_csr_gpu": (c_int, [POINTER(BSRMatrix), POINTER(CSRMatrix), c_int, POINTER(BsrBuildResult)]),
    "spmv_c_bsr_from_csr_numeric": (c_int, [POINTER(BSRMatrix), POINTER(CSRMatrix), POINTER(BsrBuildResult)]),
    "spmv_c_csr_block_count_gpu": (c_int, [POINTER(CSRMatrix), c_int, POINTER(c_int64)]),
    "spmv_c_bsr_to_csr_gpu": (c_int, [POINTER(CSRMatrix), POINTER(BSRMatrix), c_int]),
    "spmv_c_bsr_to_csr_cpu": (c_int, [POINTER(CSRMatrix), POINTER(BSRMatrix), c_int]),
    "spmv_c_cpu_bsr": (None, [POINTER(BSRMatrix), c_void_p, c_void_p]),
    "spmv_c_spmv_bsr": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int,
                                POINTER(SpMVResult)]),
    "spmv_c_spmv_bsr_async": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(SpMVConfig), c_int, c_void_p]),
    "spmv_c_compute_bandwidth_bsr": (c_int, [POINTER(BSRMatrix), c_float, POINTER(BandwidthMetrics)]),
    "spmv_c_bsr_diag_inverse_cpu": (c_int, [POINTER(BSRMatrix), c_void_p]),
    "spmv_c_bsr_diag_inverse_gpu": (c_int, [POINTER(BSRMatrix), c_void_p]),
    "spmv_c_bsr_diag_apply_cpu": (None, [POINTER(BSRMatrix), c_void_p, c_void_p, c_void_p]),
    "spmv_c_bsr_diag_apply": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, c_void_p]),
    "spmv_c_cg_solve_bsr": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(CGConfig), POINTER(CGResult)]),
    "spmv_c_bsr_ic0_cpu": (c_int, [POINTER(BSRMatrix), c_void_p, POINTER(c_int32)]),
    "spmv_c_bsr_ic0": (c_int, [POINTER(BSRMatrix), c_void_p, POINTER(IC0Result)]),
    "spmv_c_bsr_ic0_async": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p]),
    "spmv_c_sptrsv_cpu_bsr": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig)]),
    "spmv_c_sptrsv_bsr": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig),
                          POINTER(SpTRSVResult)]),
    "spmv_c_sptrsv_bsr_async": (c_int, [POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(SpTRSVConfig), c_void_p]),
    "spmv_c_sptrsv_analyze_bsr": (c_int, [POINTER(BSRMatrix), c_int, POINTER(SpTRSVResult)]),
    "spmv_c_cg_solve_bsr_ic": (c_int, [POINTER(BSRMatrix), POINTER(BSRMatrix), c_void_p, c_void_p, POINTER(CGConfig),
                               POINTER(CGResult)]),
    "spmv_c_csr_scale_gpu": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, c_void_p]),
    "spmv_c_csr_scale_cpu": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, c_void_p]),
    "spmv_c_csr_diagonal_gpu": (c_int, [POINTER(CSRMatrix), c_void_p]),
    "spmv_c_csr_diagonal_cpu": (c_int, [POINTER(CSRMatrix), c_void_p]),
    "spmv_c_csr_diag_matrix_gpu": (c_int, [POINTER(CSRMatrix), c_int, c_void_p]),
    "spmv_c_csr_diag_matrix_cpu": (c_int, [POINTER(CSRMatrix), c_int, c_void_p]),
    "spmv_c_compute_bandwidth_csr": (c_int, [POINTER(CSRMatrix), c_float, POINTER(BandwidthMetrics)]),
    "spmv_c_compute_bandwidth_csr_multi": (c_int, [POINTER(CSRMatrix), c_int, c_float, POINTER(BandwidthMetrics)]),
    "spmv_c_compute_bandwidth_ell": (c_int, [POINTER(ELLMatrix), c_float, POINTER(BandwidthMetrics)]),
    "spmv_c_get_gpu_peak_bandwidth": (c_float, []),
    "spmv_c_pagerank": (c_int, [POINTER(CSRMatrix), POINTER(PageRankConfig), POINTER(_PageRankResultC)]),
    "spmv_c_pagerank_free": (None, [POINTER(_PageRankResultC)]),
    "spmv_c_pagerank_top_k": (None, [POINTER(_PageRankResultC), c_int, c_int, POINTER(TopKNode)]),
    "spmv_c_pagerank_multi_gpu": (c_int, [POINTER(CSRMatrix), POINTER(PageRankConfig), c_int, POINTER(_PageRankResultC)]),
    "spmv_c_pagerank_shard_bounds": (c_int, [POINTER(c_int32), c_int, c_int, POINTER(c_int32)]),
    "spmv_c_pagerank_personalized": (c_int, [POINTER(CSRMatrix), c_void_p, c_int, c_void_p, c_int, c_int,
                                             POINTER(PageRankConfig), POINTER(PersonalizedResult)]),
    "spmv_c_pagerank_personalized_seeds": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p, c_int, c_void_p, c_int,
                                                   POINTER(PageRankConfig), POINTER(PersonalizedResult)]),
    "spmv_c_pr_shard_create": (c_void_p, [POINTER(CSRMatrix), c_int, c_int, c_void_p]),
    "spmv_c_pr_shard_create_chunked": (c_void_p, [POINTER(CSRMatrix), c_int, c_int, c_int, c_int, c_void_p]),
    "spmv_c_pr_shard_destroy": (None, [c_void_p]),
    "spmv_c_pr_expand": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "spmv_c_pr_reset": (c_int, [c_void_p, c_float, c_void_p]),
    "spmv_c_pr_step": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p]),
    "spmv_c_pr_step_commit": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p]),
    "spmv_c_pr_step_push": (c_int, [c_void_p, c_void_p, c_void_p, c_float, POINTER(c_void_p), c_int, c_void_p]),
    "spmv_c_pr_reduce": (c_int, [c_void_p, c_void_p, c_void_p]),
    "spmv_c_pr_commit": (c_int, [c_void_p, c_void_p, c_float, c_void_p]),
    "spmv_c_pr_reduce_commit": (c_int, [c_void_p, c_float, c_void_p]),
    "spmv_c_pr_commit_gathered": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_float, c_void_p]),
    "spmv_c_pr_status_get": (c_int, [c_void_p, POINTER(PrStatus), c_void_p]),
    "spmv_c_pr_column_sums": (c_int, [POINTER(CSRMatrix), c_void_p, c_void_p]),
    "spmv_c_pr_mask_from_column_sums": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_fill": (c_int, [c_void_p, c_size_t, c_float, c_void_p]),
    "spmv_c_gen_uniform_rows": (c_int, [c_uint64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "spmv_c_gen_uniform_ell": (c_int, [c_uint64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "spmv_c_gen_stratified_rows": (c_int, [c_uint64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "spmv_c_gen_vector": (c_int, [c_uint64, c_uint64, c_size_t, c_void_p, c_void_p]),
    "spmv_c_count_columns": (c_int, [c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "spmv_c_reciprocal_values": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _share_torchs_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same soname,
    libamdhip64.so.7, loaded by path); if libspmv_amd.so pulled in /opt/rocm's copy first, a later
    `import torch` would bring up a second runtime that finds no GPU.  So when torch is installed,
    its copy is loaded first (without importing torch) and libspmv_amd.so binds to it by soname —
    the same pairing that results when torch happens to be imported first."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    candidate = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(candidate):
        try:
            ctypes.CDLL(candidate, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> ctypes.CDLL:
    """The loaded libspmv_amd.so; raises LibraryNotBuilt when it is missing."""
    global _lib
    if _lib is None:
        _share_torchs_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise LibraryNotBuilt(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                f"(or `make -C gpu-spmv_amd`).  There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _SIGNATURES.items():
            fn = getattr(handle, name)   # AttributeError here = header / library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def version() -> str:
    return lib().spmv_c_version().decode()


def device_count() -> int:
    return lib().spmv_c_device_count()


def device_name() -> str:
    buf = ctypes.create_string_buffer(256)
    lib().spmv_c_device_name(buf, 256)
    return buf.value.decode()


def require_gpu() -> None:
    if device_count() < 1:
        raise RuntimeError("gpu-spmv_amd: no HIP device visible; the SpMV path has no CPU fallback")


def spmv_error_string(code: int) -> str:
    return lib().spmv_c_error_string(int(code)).decode()


def set_stream(stream_handle) -> None:
    lib().spmv_c_set_stream(c_void_p(stream_handle))


def device_synchronize() -> None:
    lib().spmv_c_device_synchronize()


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(c_void_p)


_NP_BY_NAME = {"float": np.float32, "float32": np.float32, "int": np.int32, "int32": np.int32,
               "double": np.float64, "float64": np.float64, "uint8": np.uint8, "int64": np.int64,
               "uint64": np.uint64}


class CudaBuffer:
    """RAII device buffer — reference include/spmv/cuda_buffer.h:12-101.

    Same behaviour: sized construction allocates in HBM (CudaException on failure),
    copies raise RuntimeError("Copy size exceeds buffer size") when count > size,
    resize discards contents, zero size holds a null pointer, move-only.
    """

    def __init__(self, count: int = 0, dtype="float32"):
        self._dtype = np.dtype(_NP_BY_NAME.get(dtype, dtype))
        self._ptr = c_void_p(None)
        self._size = 0
        if count:
            self._allocate(int(count))

    def _allocate(self, count: int) -> None:
        self._size = count
        if count > 0:
            ptr = c_void_p(None)
            status = lib().spmv_c_device_malloc(byref(ptr), count * self._dtype.itemsize)
            if status != 0:
                self._size = 0
                raise CudaException("CUDA error: " + spmv_error_string(status))
            self._ptr = ptr

    def get(self):
        """device address (int) or None"""
        return self._ptr.value

    def size(self) -> int:
        return self._size

    def empty(self) -> bool:
        return self._ptr.value is None or self._size == 0

    def copyFromHost(self, host_data, count: int) -> None:
        if count > self._size:
            raise RuntimeError("Copy size exceeds buffer size")
        src = np.ascontiguousarray(host_data, dtype=self._dtype)
        status = lib().spmv_c_memcpy_h2d(self._ptr, _np_ptr(src), int(count) * self._dtype.itemsize)
        if status != 0:
            raise CudaException("CUDA error: " + spmv_error_string(status))

    def copyToHost(self, count: int = None) -> np.ndarray:
        if count is None:
            count = self._size
        if count > self._size:
            raise RuntimeError("Copy size exceeds buffer size")
        out = np.empty(count, dtype=self._dtype)
        status = lib().spmv_c_memcpy_d2h(_np_ptr(out), self._ptr, int(count) * self._dtype.itemsize)
        if status != 0:
            raise CudaException("CUDA error: " + spmv_error_string(status))
        return out

    def resize(self, new_count: int) -> None:
        if new_count == self._size:
            return
        self.release()
        self._allocate(int(new_count))

    def release(self) -> None:
        if self._ptr.value is not None:
            lib().spmv_c_device_free(self._ptr)
            self._ptr = c_void_p(None)
        self._size = 0

    def move(self) -> "CudaBuffer":
        """C++ move construction: the returned buffer owns the allocation, self is emptied."""
        other = CudaBuffer(0, self._dtype)
        other._ptr, other._size = self._ptr, self._size
        self._ptr, self._size = c_void_p(None), 0
        return other

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


# ---- CSR container (reference include/spmv/csr_matrix.h:31-71) ---------------------
def csr_create(rows, cols, nnz):
    p = lib().spmv_c_csr_create(rows, cols, nnz)
    return p if p else None


def csr_destroy(mat) -> None:
    if mat:
        lib().spmv_c_csr_destroy(mat)


def csr_from_dense(csr, dense, rows, cols) -> int:
    if dense is None:
        return lib().spmv_c_csr_from_dense(csr, None, rows, cols)
    d = np.ascontiguousarray(dense, dtype=np.float32)
    return lib().spmv_c_csr_from_dense(csr, _np_ptr(d), rows, cols)


def csr_to_dense(csr) -> np.ndarray:
    m = csr.contents
    out = np.empty((m.num_rows, m.num_cols), dtype=np.float32)
    status = lib().spmv_c_csr_to_dense(csr, _np_ptr(out))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return out


def csr_get_element(mat, row, col) -> float:
    return float(lib().spmv_c_csr_get_element(mat, row, col))


def csr_to_gpu(mat) -> int:
    return lib().spmv_c_csr_to_gpu(mat)


def csr_from_gpu(mat) -> int:
    return lib().spmv_c_csr_from_gpu(mat)


def csr_free_gpu(mat) -> None:
    lib().spmv_c_csr_free_gpu(mat)


def csr_invalidate_gpu_cache(mat) -> None:
    """After writing into the matrix's device arrays in place: drop the cached plan / tables."""
    lib().spmv_c_csr_invalidate_gpu_cache(mat)


def csr_serialize(mat, filename) -> int:
    return lib().spmv_c_csr_serialize(mat, os.fsencode(filename) if filename is not None else None)


def csr_deserialize(mat, filename) -> int:
    return lib().spmv_c_csr_deserialize(mat, os.fsencode(filename) if filename is not None else None)


def csr_compute_stats(mat) -> CSRStats:
    out = CSRStats()
    lib().spmv_c_csr_compute_stats(mat, byref(out))
    return out


def csr_wrap_device(rows, cols, nnz, d_row_ptrs, d_col_indices, d_values):
    """Header over caller-owned device arrays (e.g. torch tensors' data_ptr())."""
    p = lib().spmv_c_csr_wrap_device(rows, cols, nnz, c_void_p(d_row_ptrs), c_void_p(d_col_indices),
                                     c_void_p(d_values))
    return p if p else None


def csr_from_arrays(num_rows, num_cols, row_ptrs, col_indices, values):
    """Convenience: csr_create + fill of the host arrays (what the reference's callers do by hand)."""
    row_ptrs = np.ascontiguousarray(row_ptrs, dtype=np.int32)
    col_indices = np.ascontiguousarray(col_indices, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    assert row_ptrs.size == num_rows + 1 and col_indices.size == values.size
    mat = csr_create(num_rows, num_cols, int(values.size))
    m = mat.contents
    ctypes.memmove(m.row_ptrs, _np_ptr(row_ptrs), row_ptrs.nbytes)
    if values.size:
        ctypes.memmove(m.col_indices, _np_ptr(col_indices), col_indices.nbytes)
        ctypes.memmove(m.values, _np_ptr(values), values.nbytes)
    return mat


def csr_host_arrays(mat):
    """(row_ptrs, col_indices, values) numpy copies of the host arrays."""
    m = mat.contents
    rp = np.ctypeslib.as_array(m.row_ptrs, shape=(m.num_rows + 1,)).copy()
    if m.nnz > 0:
        ci = np.ctypeslib.as_array(m.col_indices, shape=(m.nnz,)).copy()
        va = np.ctypeslib.as_array(m.values, shape=(m.nnz,)).copy()
    else:
        ci, va = np.empty(0, np.int32), np.empty(0, np.float32)
    return rp, ci, va


# ---- ELL container (reference include/spmv/ell_matrix.h:31-66) ---------------------
def ell_create(rows, cols, max_nnz_per_row):
    p = lib().spmv_c_ell_create(rows, cols, max_nnz_per_row)
    return p if p else None


def ell_destroy(mat) -> None:
    if mat:
        lib().spmv_c_ell_destroy(mat)


def ell_from_dense(ell, dense, rows, cols) -> int:
    if dense is None:
        return lib().spmv_c_ell_from_dense(ell, None, rows, cols)
    d = np.ascontiguousarray(dense, dtype=np.float32)
    return lib().spmv_c_ell_from_dense(ell, _np_ptr(d), rows, cols)


def ell_from_csr(ell, csr) -> int:
    return lib().spmv_c_ell_from_csr(ell, csr)


def csr_transpose_gpu(AT, A) -> int:
    """Extension: AT = A^T built on the device, deterministic (csr_matrix.h csr_transpose_gpu); csr_from_gpu(AT)
    fills AT's host arrays."""
    return lib().spmv_c_csr_transpose_gpu(AT, A)


def fsai_csr(G, A, S=None) -> FSAIResult:
    """G = FSAI of the square device matrix A on the lower pattern of S (None: A) (include/spmv/fsai.h fsai_csr),
    bit-identical to fsai_cpu_csr; G owns new device arrays afterwards and csr_from_gpu(G) fills its host arrays.
    result.error_code is the return value."""
    out = FSAIResult()
    out.error_code = lib().spmv_c_fsai_csr(G, A, S, byref(out))
    return out


def fsai_csr_numeric(G, A) -> FSAIResult:
    """Only G's device values again from a new A, on the pattern an earlier fsai_csr produced (fsai.h
    fsai_csr_numeric)."""
    out = FSAIResult()
    out.error_code = lib().spmv_c_fsai_csr_numeric(G, A, byref(out))
    return out


def fsai_cpu_csr(G, A, S=None):
    """The same operation on host arrays, the definition of the arithmetic (fsai.h fsai_cpu_csr); G gets new host
    arrays (csr_host_arrays(G) reads them).  Returns (status, bad_row)."""
    bad = c_int32(-1)
    status = lib().spmv_c_fsai_cpu_csr(G, A, S, byref(bad))
    return status, bad.value


def spgemm_csr(C, A, B) -> SpGEMMResult:
    """C = A*B of two device matrices (include/spmv/spgemm.h spgemm_csr), bit-identical to spgemm_cpu_csr; C owns new
    device arrays afterwards and csr_from_gpu(C) fills its host arrays.  result.error_code is the return value."""
    out = SpGEMMResult()
    out.error_code = lib().spmv_c_spgemm_csr(C, A, B, byref(out))
    return out


def spgemm_csr_numeric(C, A, B) -> SpGEMMResult:
    """Only C's device values again, into the pattern an earlier spgemm_csr produced (spgemm.h spgemm_csr_numeric)."""
    out = SpGEMMResult()
    out.error_code = lib().spmv_c_spgemm_csr_numeric(C, A, B, byref(out))
    return out


def spgemm_cpu_csr(C, A, B) -> int:
    """The product on host arrays, the definition of the arithmetic (spgemm.h spgemm_cpu_csr); C gets new host
    arrays (csr_host_arrays(C) reads them)."""
    return lib().spmv_c_spgemm_cpu_csr(C, A, B)


def spgemm_class_capacity(cls) -> int:
    """Most distinct columns of a row in accumulator class cls (1-based); INT_MAX for the dense class, -1 past it."""
    return lib().spmv_c_spgemm_class_capacity(int(cls))


def ell_from_csr_gpu(ell, csr) -> int:
    """Extension: CSR -> ELL on the device (device slabs only; ell_from_gpu mirrors them to the host)."""
    return lib().spmv_c_ell_from_csr_gpu(ell, csr)


def ell_to_dense(ell) -> np.ndarray:
    m = ell.contents
    out = np.empty((m.num_rows, m.num_cols), dtype=np.float32)
    status = lib().spmv_c_ell_to_dense(ell, _np_ptr(out))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return out


def ell_get_element(mat, row, col) -> float:
    return float(lib().spmv_c_ell_get_element(mat, row, col))


def ell_to_gpu(mat) -> int:
    return lib().spmv_c_ell_to_gpu(mat)


def ell_from_gpu(mat) -> int:
    return lib().spmv_c_ell_from_gpu(mat)


def ell_free_gpu(mat) -> None:
    lib().spmv_c_ell_free_gpu(mat)


def ell_invalidate_gpu_cache(mat) -> None:
    lib().spmv_c_ell_invalidate_gpu_cache(mat)


def ell_serialize(mat, filename) -> int:
    return lib().spmv_c_ell_serialize(mat, os.fsencode(filename) if filename is not None else None)


def ell_deserialize(mat, filename) -> int:
    return lib().spmv_c_ell_deserialize(mat, os.fsencode(filename) if filename is not None else None)


def ell_index(row, k, num_rows) -> int:
    return lib().spmv_c_ell_index(row, k, num_rows)


def ell_wrap_device(rows, cols, max_nnz_per_row, d_col_indices, d_values):
    p = lib().spmv_c_ell_wrap_device(rows, cols, max_nnz_per_row, c_void_p(d_col_indices), c_void_p(d_values))
    return p if p else None


def ell_host_arrays(mat):
    m = mat.contents
    slots = m.num_rows * m.max_nnz_per_row
    if slots == 0:
        return np.empty(0, np.int32), np.empty(0, np.float32)
    ci = np.ctypeslib.as_array(m.col_indices, shape=(slots,)).copy()
    va = np.ctypeslib.as_array(m.values, shape=(slots,)).copy()
    return ci, va


# ---- SpMV (reference include/spmv/spmv.h:39-54) -------------------------------------
def spmv_cpu_csr(A, x) -> np.ndarray:
    """The library's host path (reference API parity); not used by any device entry point."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros(A.contents.num_rows, dtype=np.float32)
    lib().spmv_c_cpu_csr(A, _np_ptr(x), _np_ptr(y))
    return y


def spmv_cpu_ell(A, x) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros(A.contents.num_rows, dtype=np.float32)
    lib().spmv_c_cpu_ell(A, _np_ptr(x), _np_ptr(y))
    return y


def _dev(ptr):
    if isinstance(ptr, CudaBuffer):
        return c_void_p(ptr.get())
    return c_void_p(ptr)


def spmv_csr(A, d_x, d_y, config=None, vec_size=-1) -> SpMVResult:
    out = SpMVResult()
    lib().spmv_c_spmv_csr(A, _dev(d_x), _dev(d_y), byref(config) if config is not None else None,
                          vec_size, byref(out))
    return out


def spmv_ell(A, d_x, d_y, config=None, vec_size=-1) -> SpMVResult:
    out = SpMVResult()
    lib().spmv_c_spmv_ell(A, _dev(d_x), _dev(d_y), byref(config) if config is not None else None,
                          vec_size, byref(out))
    return out


def csr_tiled_checksum(A):
    """Four position-weighted checksums of the matrix's tiled plan (values, local columns, row deltas, cell
    table), or None without a plan."""
    out = (c_uint64 * 4)()
    if not lib().spmv_c_csr_tiled_checksum(A, out):
        return None
    return tuple(int(v) for v in out)


def csr_has_tiled_plan(A) -> bool:
    return bool(lib().spmv_c_csr_has_tiled_plan(A))


def set_tiled_promotion(calls: int) -> None:
    """spmv_set_tiled_promotion (include/spmv/spmv.h): VECTOR_CSR / MERGE_PATH callers without use_texture move to the
    LDS-tiled engine after `calls` calls on a large matrix; 0 = never."""
    lib().spmv_c_set_tiled_promotion(int(calls))


def get_tiled_promotion() -> int:
    return int(lib().spmv_c_get_tiled_promotion())


def tiled_shape(rows, cols, nnz):
    """(takes_it, strip_cols, tile_rows) the LDS-tiled engine would use for such a matrix."""
    w, r = c_int32(0), c_int32(0)
    takes = lib().spmv_c_tiled_shape(rows, cols, nnz, byref(w), byref(r))
    return bool(takes), w.value, r.value


def csr_tiled_info(A):
    """dict describing the matrix's cached tiled plan, or None."""
    out = (c_int64 * 8)()
    if not lib().spmv_c_csr_tiled_info(A, out):
        return None
    keys = ("strip_cols", "tile_rows", "num_strips", "num_tiles", "slots_in_cells", "long_rows",
            "slots_per_lane", "long_row_limit")
    info = dict(zip(keys, (int(v) for v in out)))
    info["values_folded"] = bool(lib().spmv_c_csr_tiled_folded(A))
    stats = (c_double * 4)()
    if lib().spmv_c_csr_tiled_stats(A, stats):
        info["build_ms"] = round(float(stats[0]), 3)
        info["plan_bytes"] = int(stats[1])
        info["entries_in_cells"] = int(stats[3])
    # the local columns as the plan holds them; plan_bytes counts them at two bytes a slot either way
    info["col_bytes"] = int(lib().spmv_c_csr_tiled_col_bytes(A))
    return info


def csr_tiled_items(A) -> int:
    """Number of phase-1 work items of the matrix's cached tiled plan, or -1 without a plan."""
    return int(lib().spmv_c_csr_tiled_items(A))


_PLAN_INFO10 = ("strip_cols", "tile_rows", "num_strips", "num_tiles", "slots_in_cells", "long_rows", "slots_per_lane",
                "long_row_limit", "values_folded", "num_items")


def _plan_info10(call, handle):
    out = (c_int64 * 10)()
    if not call(handle, out):
        return None
    info = dict(zip(_PLAN_INFO10, (int(v) for v in out)))
    info["values_folded"] = bool(info["values_folded"])
    return info


def ell_tiled_info(E):
    """dict describing the tiled plan built from the ELL matrix's slabs (spmv_ell with use_texture), or None."""
    return _plan_info10(lib().spmv_c_ell_tiled_info, E)


def csr_transpose_tiled_info(A):
    """dict describing the tiled plan owned by A's cached transpose (spmv_csr_transpose with use_texture), or None."""
    return _plan_info10(lib().spmv_c_csr_transpose_tiled_info, A)


def spmv_csr_async(A, d_x, d_y, config=None, vec_size=-1, stream=None) -> int:
    return lib().spmv_c_spmv_csr_async(A, _dev(d_x), _dev(d_y),
                                       byref(config) if config is not None else None, vec_size,
                                       c_void_p(stream))


def spmv_ell_async(A, d_x, d_y, config=None, vec_size=-1, stream=None) -> int:
    return lib().spmv_c_spmv_ell_async(A, _dev(d_x), _dev(d_y),
                                       byref(config) if config is not None else None, vec_size,
                                       c_void_p(stream))


def spmv_csr_multi(A, d_X, d_Y, k, ldx=None, ldy=None, config=None, vec_size=-1) -> SpMVResult:
    """Y = A * X for k right-hand sides (include/spmv/spmv.h spmv_csr_multi): X num_cols x k and Y num_rows x k,
    row-major device arrays with leading dimensions ldx, ldy (default k); Y's columns k..ldy-1 are never written."""
    out = SpMVResult()
    ldx = k if ldx is None else ldx
    ldy = k if ldy is None else ldy
    lib().spmv_c_spmv_csr_multi(A, _dev(d_X), int(ldx), _dev(d_Y), int(ldy), int(k),
                                byref(config) if config is not None else None, vec_size, byref(out))
    return out


def spmv_csr_multi_async(A, d_X, d_Y, k, ldx=None, ldy=None, config=None, vec_size=-1, stream=None) -> int:
    ldx = k if ldx is None else ldx
    ldy = k if ldy is None else ldy
    return lib().spmv_c_spmv_csr_multi_async(A, _dev(d_X), int(ldx), _dev(d_Y), int(ldy), int(k),
                                             byref(config) if config is not None else None, vec_size,
                                             c_void_p(stream))


def spmv_csr_transpose(A, d_x, d_y, config=None, vec_size=-1) -> SpMVResult:
    """y = A^T * x (include/spmv/spmv.h spmv_csr_transpose): d_x has num_rows entries, d_y num_cols; the first call
    on a matrix builds and caches its device transpose."""
    out = SpMVResult()
    lib().spmv_c_spmv_csr_transpose(A, _dev(d_x), _dev(d_y), byref(config) if config is not None else None,
                                    vec_size, byref(out))
    return out


def spmv_csr_transpose_async(A, d_x, d_y, config=None, vec_size=-1, stream=None) -> int:
    return lib().spmv_c_spmv_csr_transpose_async(A, _dev(d_x), _dev(d_y),
                                                 byref(config) if config is not None else None, vec_size,
                                                 c_void_p(stream))


def cg_solve(A, d_b, d_x, config=None) -> CGResult:
    """Preconditioned CG for A x = b on the device (include/spmv/cg.h cg_solve): d_b and d_x hold num_rows floats,
    d_x is the initial guess on entry and the solution on exit."""
    out = CGResult()
    lib().spmv_c_cg_solve(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def cg_solve_multi(A, d_B, d_X, k, ldb=None, ldx=None, config=None) -> list:
    """cg_solve for k right-hand sides in one matrix pass per step (include/spmv/cg.h cg_solve_multi): d_B and d_X
    are num_rows x k row-major with leading dimensions ldb, ldx >= k (default k); returns one CGResult per column
    (at least one, so that a rejected call always has somewhere to report its error_code)."""
    k = int(k)
    ldb = k if ldb is None else int(ldb)
    ldx = k if ldx is None else int(ldx)
    out = (CGResult * max(k, 1))()
    rc = lib().spmv_c_cg_solve_multi(A, _dev(d_B), ldb, _dev(d_X), ldx, k,
                                     byref(config) if config is not None else None, out)
    results = list(out)
    if rc != 0:
        for r in results:
            r.error_code = rc
    return results


def bicgstab_solve(A, d_b, d_x, config=None) -> BiCGStabResult:
    """Jacobi-preconditioned BiCGSTAB for a square non-singular A x = b on the device (include/spmv/bicgstab.h
    bicgstab_solve): d_b and d_x hold num_rows floats, d_x is the initial guess on entry and the solution on exit."""
    out = BiCGStabResult()
    lib().spmv_c_bicgstab_solve(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                byref(out))
    return out


def bicgstab_solve_lu(A, LU, d_b, d_x, config=None) -> BiCGStabResult:
    """BiCGSTAB right-preconditioned by M = L U, the unit lower and the upper triangle of the device matrix LU
    (include/spmv/bicgstab.h bicgstab_solve_lu); LU is usually ilu0_csr's output wrapped by csr_wrap_device over A's
    structure arrays.  config.preconditioner is not read."""
    out = BiCGStabResult()
    lib().spmv_c_bicgstab_solve_lu(A, LU, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                   byref(out))
    return out


def gmres_solve(A, d_b, d_x, config=None) -> GMRESResult:
    """Restarted GMRES(m) for a square non-singular A x = b on the device (include/spmv/gmres.h gmres_solve): d_b and
    d_x hold num_rows floats, d_x is the initial guess on entry and the solution on exit; relative_residual and
    converged come from the recomputed b - A x."""
    out = GMRESResult()
    lib().spmv_c_gmres_solve(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def gmres_solve_lu(A, LU, d_b, d_x, config=None) -> GMRESResult:
    """GMRES(m) right-preconditioned by M = L U, the unit lower and the upper triangle of the device matrix LU
    (include/spmv/gmres.h gmres_solve_lu); LU is usually ilu0_csr's output wrapped by csr_wrap_device over A's
    structure arrays.  config.preconditioner is not read."""
    out = GMRESResult()
    lib().spmv_c_gmres_solve_lu(A, LU, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                byref(out))
    return out


def minres_solve(A, d_b, d_x, config=None) -> MinresResult:
    """Preconditioned MINRES for (A - shift I) x = b, A square and symmetric, definite or not, on the device
    (include/spmv/minres.h minres_solve): d_b and d_x hold num_rows floats, d_x is the initial guess on entry and the
    solution on exit.  relative_residual and converged are the recurrence's (M^-1-norm); true_relative_residual is
    recomputed from the returned x."""
    out = MinresResult()
    lib().spmv_c_minres_solve(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def minres_solve_ic(A, F, d_b, d_x, config=None) -> MinresResult:
    """MINRES preconditioned by M = L L^T, the lower and the upper triangle of the device factor matrix F
    (include/spmv/minres.h minres_solve_ic); F is usually ic0_csr's output for an SPD sibling of A, wrapped by
    csr_wrap_device.  config.preconditioner is not read."""
    out = MinresResult()
    lib().spmv_c_minres_solve_ic(A, F, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                 byref(out))
    return out


def eigs_sym(A, d_values, d_vectors, ldv=None, d_residuals=None, d_v0=None, config=None) -> EigsResult:
    """config.num_values eigenpairs at one end of the spectrum of the symmetric device matrix A by thick-restart
    Lanczos (include/spmv/eigs.h eigs_sym): d_values holds num_values floats, vector i is num_rows floats at
    d_vectors + i * ldv (ldv None = num_rows), d_residuals (optional) num_values floats, d_v0 (optional) the start
    vector; all device pointers or CudaBuffers."""
    out = EigsResult()
    lib().spmv_c_eigs_sym(A, _dev(d_values), _dev(d_vectors), A.num_rows if ldv is None else int(ldv),
                          _dev(d_residuals), _dev(d_v0), byref(config) if config is not None else None, byref(out))
    return out


def sym_eig_small(T, on_device=False):
    """Eigen-decomposition of the dense symmetric fp64 matrix T (order <= 64) by the fixed Jacobi rule of
    include/spmv/eigs.h: (error code, values ascending, vectors with eigenvector i in ROW i).  on_device runs the
    one-workgroup device kernel; both forms give the same bits."""
    T = np.ascontiguousarray(T, np.float64)
    n = T.shape[0]
    values = np.zeros(n, np.float64)
    vectors = np.zeros((n, n), np.float64)
    status = lib().spmv_c_sym_eig_small(n, _np_ptr(T), n, _np_ptr(values), _np_ptr(vectors), 1 if on_device else 0)
    return status, values, vectors


def ilu0_csr(A, d_lu_values) -> ILU0Result:
    """ILU(0) of the square device matrix A into d_lu_values (include/spmv/ilu0.h ilu0_csr): nnz floats in A's
    pattern, L left of the diagonal, U on and right of it; d_lu_values may be A's own device values (in place)."""
    out = ILU0Result()
    lib().spmv_c_ilu0_csr(A, _dev(d_lu_values), byref(out))
    return out


def ilu0_csr_async(A, d_lu_values, stream=None) -> int:
    return lib().spmv_c_ilu0_csr_async(A, _dev(d_lu_values), c_void_p(stream))


def ilu0_cpu_csr(A):
    """The factorisation on A's host arrays (include/spmv/ilu0.h ilu0_cpu_csr, the definition of the arithmetic):
    returns (lu_values, zero_pivot); raises ValueError with the library's error string when the call is rejected."""
    lu = np.zeros(max(int(A.contents.nnz), 0) if A else 0, dtype=np.float32)
    pivot = c_int32(-1)
    status = lib().spmv_c_ilu0_cpu_csr(A, _np_ptr(lu), byref(pivot))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return lu, pivot.value


def cg_solve_ic(A, F, d_b, d_x, config=None) -> CGResult:
    """CG preconditioned by M = L L^T, L the lower and L^T the upper triangle of the device matrix F
    (include/spmv/cg.h cg_solve_ic); F is usually ic0_csr's output wrapped by csr_wrap_device over A's structure
    arrays.  config.preconditioner is not read."""
    out = CGResult()
    lib().spmv_c_cg_solve_ic(A, F, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def amg_setup(A, config=None, aggregates=None):
    """(AMGResult, hierarchy handle or None): the aggregation AMG hierarchy of the device matrix A (include/spmv/amg.h
    amg_setup).  aggregates: None, or a list of int32 arrays, aggregates[l][i] = the aggregate of row i of level l.
    Release the handle with amg_destroy."""
    out, handle = AMGResult(), c_void_p()
    maps, table = None, None
    if aggregates is not None:
        maps = [np.ascontiguousarray(a, dtype=np.int32) for a in aggregates]
        table = (c_void_p * max(len(maps), 1))(*[a.ctypes.data for a in maps])
    lib().spmv_c_amg_setup(byref(handle), A, byref(config) if config is not None else None,
                           len(maps) if maps is not None else 0, table, byref(out))
    return out, (handle.value if handle.value else None)


def amg_update(H, A) -> AMGResult:
    """New values in the same pattern: every level of H refilled, the aggregates kept (amg.h amg_update)."""
    out = AMGResult()
    lib().spmv_c_amg_update(H, A, byref(out))
    return out


def amg_destroy(H) -> None:
    if H:
        lib().spmv_c_amg_destroy(H)


def amg_num_levels(H) -> int:
    return lib().spmv_c_amg_num_levels(H)


def amg_level(H, level):
    """(status, view, d_aggregate, num_aggregates): level `level` of H as a CSRMatrix header over device arrays that
    owns nothing (a ctypes structure, not a pointer), the device address of its aggregate map (None on the coarsest
    level) and the number of aggregates."""
    view, d_agg, count = CSRMatrix(), c_void_p(), c_int32(0)
    status = lib().spmv_c_amg_level(H, int(level), byref(view), byref(d_agg), byref(count))
    return status, view, d_agg.value, count.value


def amg_level_arrays(H, level):
    """(n, row_ptrs, col_indices, values, aggregate or None): numpy copies of level `level` of H, read back from the
    device."""
    status, view, d_agg, _ = amg_level(H, level)
    if status != 0:
        raise ValueError(spmv_error_string(status))

    def down(ptr, count, dtype):
        host = np.empty(count, dtype)
        if count and lib().spmv_c_memcpy_d2h(_np_ptr(host), c_void_p(ptr), host.nbytes) != 0:
            raise CudaException("device-to-host copy failed")
        return host

    n, nnz = view.num_rows, view.nnz
    cast = lambda p: ctypes.cast(p, c_void_p).value
    rp = down(cast(view.d_row_ptrs), n + 1, np.int32)
    ci = down(cast(view.d_col_indices), nnz, np.int32)
    va = down(cast(view.d_values), nnz, np.float32)
    return n, rp, ci, va, (down(d_agg, n, np.int32) if d_agg else None)


def amg_apply(H, d_r, d_z) -> int:
    """d_z = one V-cycle of H on d_r from a zero guess (amg.h amg_apply)."""
    return lib().spmv_c_amg_apply(H, _dev(d_r), _dev(d_z))


def amg_aggregate_cpu_csr(A, strength=0.08):
    """(status, aggregate int32[num_rows], count): the aggregation of one level on A's host arrays, the definition
    (amg.h amg_aggregate_cpu_csr)."""
    agg = np.full(max(A.contents.num_rows, 0), -7, np.int32)
    count = c_int32(-7)
    status = lib().spmv_c_amg_aggregate_cpu_csr(A, float(strength), _np_ptr(agg), byref(count))
    return status, agg, count.value


def amg_aggregate_mis2_cpu_csr(A, strength=0.08, seed=0):
    """(status, aggregate int32[num_rows], count, rounds): the MIS-2 aggregation of one level on A's host arrays, the
    definition of the device's (amg.h amg_aggregate_mis2_cpu_csr); -1 marks a vertex left free, rounds is the
    synchronous round count."""
    agg = np.full(max(A.contents.num_rows, 0), -7, np.int32)
    count, rounds = c_int32(-7), c_int32(-7)
    status = lib().spmv_c_amg_aggregate_mis2_cpu_csr(A, float(strength), int(seed) & 0xFFFFFFFF, _np_ptr(agg),
                                                     byref(count), byref(rounds))
    return status, agg, count.value, rounds.value


def amg_aggregate_mis2_gpu(A, d_aggregate, strength=0.08, seed=0):
    """(status, count, rounds): the same ints into d_aggregate, num_rows ints on the device (a device address or an
    object _dev understands) (amg.h amg_aggregate_mis2_gpu)."""
    count, rounds = c_int32(-7), c_int32(-7)
    status = lib().spmv_c_amg_aggregate_mis2_gpu(A, float(strength), int(seed) & 0xFFFFFFFF, _dev(d_aggregate),
                                                 byref(count), byref(rounds))
    return status, count.value, rounds.value


def amg_setup_device(A, config=None, seed=0):
    """(AMGResult, hierarchy handle or None): amg_setup with every level made on the device, aggregated by the MIS-2
    rule with `seed` (amg.h amg_setup_device).  Release the handle with amg_destroy."""
    out, handle = AMGResult(), c_void_p()
    lib().spmv_c_amg_setup_device(byref(handle), A, byref(config) if config is not None else None,
                                  int(seed) & 0xFFFFFFFF, byref(out))
    return out, (handle.value if handle.value else None)


def amg_setup_rounds(H, level) -> int:
    """Rounds the root selection of level `level` took (0: the coarsest level, or a hierarchy amg_setup built)."""
    return lib().spmv_c_amg_setup_rounds(H, int(level))


def amg_setup_smoothed(A, config=None, smoothing=None, aggregates=None):
    """(AMGResult, hierarchy handle or None): amg_setup with smoothed prolongators (amg.h amg_setup_smoothed);
    smoothing: an AMGSmoothing or None (the defaults)."""
    out, handle = AMGResult(), c_void_p()
    maps, table = None, None
    if aggregates is not None:
        maps = [np.ascontiguousarray(a, dtype=np.int32) for a in aggregates]
        table = (c_void_p * max(len(maps), 1))(*[a.ctypes.data for a in maps])
    lib().spmv_c_amg_setup_smoothed(byref(handle), A, byref(config) if config is not None else None,
                                    byref(smoothing) if smoothing is not None else None,
                                    len(maps) if maps is not None else 0, table, byref(out))
    return out, (handle.value if handle.value else None)


def amg_setup_smoothed_device(A, config=None, smoothing=None, seed=0):
    """(AMGResult, hierarchy handle or None): amg_setup_device with smoothed prolongators (amg.h
    amg_setup_smoothed_device)."""
    out, handle = AMGResult(), c_void_p()
    lib().spmv_c_amg_setup_smoothed_device(byref(handle), A, byref(config) if config is not None else None,
                                           byref(smoothing) if smoothing is not None else None,
                                           int(seed) & 0xFFFFFFFF, byref(out))
    return out, (handle.value if handle.value else None)


def amg_is_smoothed(H) -> int:
    return lib().spmv_c_amg_is_smoothed(H)


def amg_level_transfer(H, level):
    """(status, P_view, PT_view): the prolongator of level `level` and its transpose as CSRMatrix headers over device
    arrays that own nothing (amg.h amg_level_transfer)."""
    p_view, pt_view = CSRMatrix(), CSRMatrix()
    status = lib().spmv_c_amg_level_transfer(H, int(level), byref(p_view), byref(pt_view))
    return status, p_view, pt_view


def amg_prolongator_cpu_csr(P, A, aggregate, num_aggregates, weight=2.0 / 3.0) -> int:
    """P = the smoothed prolongator of one level from A's host arrays and the aggregate map, the host definition
    (amg.h amg_prolongator_cpu_csr)."""
    agg = np.ascontiguousarray(aggregate, dtype=np.int32)
    return lib().spmv_c_amg_prolongator_cpu_csr(P, A, _np_ptr(agg), int(num_aggregates), float(weight))


def amg_restrict(H, level, d_f, d_x, d_f_coarse) -> int:
    """d_f_coarse = P^T (d_f - A_l d_x) on level `level` (amg.h amg_restrict)."""
    return lib().spmv_c_amg_restrict(H, int(level), _dev(d_f), _dev(d_x), _dev(d_f_coarse))


def amg_prolong(H, level, d_e, d_x) -> int:
    """d_x += P d_e on level `level`, in place (amg.h amg_prolong)."""
    return lib().spmv_c_amg_prolong(H, int(level), _dev(d_e), _dev(d_x))


def cg_solve_amg(A, H, d_b, d_x, config=None) -> CGResult:
    """Solves A x = b by CG preconditioned with one V-cycle of the AMG hierarchy H per iteration (include/spmv/cg.h
    cg_solve_amg)."""
    out = CGResult()
    lib().spmv_c_cg_solve_amg(A, H, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def ic0_csr(A, d_l_values) -> IC0Result:
    """IC(0) of the square device matrix A into d_l_values (include/spmv/ic0.h ic0_csr): nnz floats in A's pattern,
    L on and left of the diagonal, L^T right of it; d_l_values may be A's own device values (in place)."""
    out = IC0Result()
    lib().spmv_c_ic0_csr(A, _dev(d_l_values), byref(out))
    return out


def ic0_csr_async(A, d_l_values, stream=None) -> int:
    return lib().spmv_c_ic0_csr_async(A, _dev(d_l_values), c_void_p(stream))


def ic0_cpu_csr(A):
    """The factorisation on A's host arrays (include/spmv/ic0.h ic0_cpu_csr, the definition of the arithmetic):
    returns (l_values, bad_pivot); raises ValueError with the library's error string when the call is rejected."""
    l = np.zeros(max(int(A.contents.nnz), 0) if A else 0, dtype=np.float32)
    pivot = c_int32(-1)
    status = lib().spmv_c_ic0_cpu_csr(A, _np_ptr(l), byref(pivot))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return l, pivot.value


def sptrsv_csr(A, d_b, d_x, config=None) -> SpTRSVResult:
    """Solves T x = b on the device, T the config.uplo triangle of the square matrix A (include/spmv/sptrsv.h
    sptrsv_csr): d_b and d_x hold num_rows floats and may be the same buffer (the solve in place)."""
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_csr(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def sptrsv_csr_async(A, d_b, d_x, config=None, stream=None) -> int:
    return lib().spmv_c_sptrsv_csr_async(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                         c_void_p(stream))


def sptrsv_analyze(A, uplo=0) -> SpTRSVResult:
    """Builds and caches the level schedule of A's `uplo` triangle ahead of a timed sptrsv_csr."""
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_analyze(A, int(uplo), byref(out))
    return out


def sptrsv_analyze_device(A, uplo=0) -> SpTRSVResult:
    """sptrsv_analyze with the analysis run on the device: no array of A crosses the bus (include/spmv/sptrsv.h
    sptrsv_analyze_device)."""
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_analyze_device(A, int(uplo), byref(out))
    return out


def sptrsv_schedule_get(A, uplo=0, arrays=True):
    """The cached level schedule of (A, uplo), of either origin (include/spmv/sptrsv.h sptrsv_schedule_get):
    (status, level_ptr[num_levels + 1], order[num_rows], SpTRSVScheduleInfo); (status, None, None, None) when the call
    is rejected (no schedule cached: INVALID_ARGUMENT).  arrays=False asks for the info alone."""
    info = SpTRSVScheduleInfo()
    if A is None or not arrays:
        status = lib().spmv_c_sptrsv_schedule_get(A, int(uplo), None, None, byref(info))
        return (status, None, None, info) if status == 0 else (status, None, None, None)
    rows = max(int(A.contents.num_rows), 0)
    level_ptr = np.zeros(rows + 1, dtype=np.int32)
    order = np.zeros(rows, dtype=np.int32)
    status = lib().spmv_c_sptrsv_schedule_get(A, int(uplo), _np_ptr(level_ptr), _np_ptr(order), byref(info))
    if status != 0:
        return status, None, None, None
    return status, level_ptr[:info.num_levels + 1].copy(), order, info


def sptrsv_cpu_csr(A, b, config=None) -> np.ndarray:
    """Host forward / backward substitution on A's host arrays (include/spmv/sptrsv.h sptrsv_cpu_csr): returns x;
    raises ValueError with the library's error string when the call is rejected."""
    b = np.ascontiguousarray(b, dtype=np.float32)
    x = np.zeros(A.contents.num_rows, dtype=np.float32)
    status = lib().spmv_c_sptrsv_cpu_csr(A, _np_ptr(b), _np_ptr(x), byref(config) if config is not None else None)
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return x


def sptrsv_csr_multi(A, d_B, d_X, k, ldb=None, ldx=None, config=None) -> SpTRSVResult:
    """sptrsv_csr for k right-hand sides in one launch sequence (include/spmv/sptrsv.h sptrsv_csr_multi): d_B and d_X
    are num_rows x k row-major with leading dimensions ldb, ldx >= k (default k) and may be the same buffer when
    ldb == ldx."""
    k = int(k)
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_csr_multi(A, _dev(d_B), k if ldb is None else int(ldb), _dev(d_X),
                                  k if ldx is None else int(ldx), k, byref(config) if config is not None else None,
                                  byref(out))
    return out


def sptrsv_csr_multi_async(A, d_B, d_X, k, ldb=None, ldx=None, config=None, stream=None) -> int:
    k = int(k)
    return lib().spmv_c_sptrsv_csr_multi_async(A, _dev(d_B), k if ldb is None else int(ldb), _dev(d_X),
                                               k if ldx is None else int(ldx), k,
                                               byref(config) if config is not None else None, c_void_p(stream))


def sptrsv_cpu_csr_multi(A, B, config=None) -> np.ndarray:
    """sptrsv_cpu_csr column by column on the num_rows x k host array B (include/spmv/sptrsv.h
    sptrsv_cpu_csr_multi): returns X (num_rows x k); raises ValueError with the library's error string when the call
    is rejected."""
    B = np.ascontiguousarray(B, dtype=np.float32)
    if B.ndim != 2:
        raise ValueError("B must be num_rows x k")
    k = B.shape[1]
    X = np.zeros_like(B)
    status = lib().spmv_c_sptrsv_cpu_csr_multi(A, _np_ptr(B), k, _np_ptr(X), k, k,
                                               byref(config) if config is not None else None)
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return X


def cg_solve_fsai(A, G, GT, d_b, d_x, config=None) -> CGResult:
    """CG preconditioned by M^-1 = GT G, z = GT (G r): two SpMVs per step (include/spmv/cg.h cg_solve_fsai); G is
    usually fsai_csr's output and GT its csr_transpose_gpu.  config.preconditioner is not read."""
    out = CGResult()
    lib().spmv_c_cg_solve_fsai(A, G, GT, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def cg_solve_multi_ic(A, F, d_B, d_X, k, ldb=None, ldx=None, config=None) -> list:
    """cg_solve_ic for k right-hand sides (include/spmv/cg.h cg_solve_multi_ic): cg_solve_multi's arrays and results,
    preconditioned by M = L L^T of the factor matrix F with one k-wide launch sequence per triangular solve."""
    k = int(k)
    ldb = k if ldb is None else int(ldb)
    ldx = k if ldx is None else int(ldx)
    out = (CGResult * max(k, 1))()
    rc = lib().spmv_c_cg_solve_multi_ic(A, F, _dev(d_B), ldb, _dev(d_X), ldx, k,
                                        byref(config) if config is not None else None, out)
    results = list(out)
    if rc != 0:
        for r in results:
            r.error_code = rc
    return results


def sptrsv_levels(num_rows, row_ptrs, col_indices, uplo=0):
    """The level analysis on the host (include/spmv/sptrsv.h sptrsv_levels):
    (status, level_ptr[num_levels + 1], order[num_rows], num_levels, first_missing_diagonal)."""
    rp = np.ascontiguousarray(row_ptrs, dtype=np.int32)
    ci = np.ascontiguousarray(col_indices, dtype=np.int32)
    level_ptr = np.zeros(max(int(num_rows), 0) + 1, dtype=np.int32)
    order = np.zeros(max(int(num_rows), 0), dtype=np.int32)
    levels, missing = c_int32(0), c_int32(-1)
    status = lib().spmv_c_sptrsv_levels(int(num_rows), _np_ptr(rp), _np_ptr(ci), int(uplo), _np_ptr(level_ptr),
                                        _np_ptr(order), byref(levels), byref(missing))
    if status != 0:
        return status, None, None, 0, -1
    return status, level_ptr[:levels.value + 1].copy(), order, levels.value, missing.value


# ---- multicolour reordering (include/spmv/reorder.h) ----------------------------------
def csr_color(A, d_colors, config=None) -> ColorResult:
    """Colours the graph of the square device matrix A into d_colors (num_rows int32 on the device): the same ints as
    csr_color_cpu (include/spmv/reorder.h csr_color)."""
    out = ColorResult()
    lib().spmv_c_csr_color(A, _dev(d_colors), byref(config) if config is not None else None, byref(out))
    return out


def csr_color_cpu(A, config=None):
    """The colouring on A's host arrays, the definition (reorder.h csr_color_cpu): (status, colors, num_colors, rounds)
    with rounds the synchronous round count; colors is None when the call fails."""
    n = max(A.contents.num_rows, 0) if A else 0
    colors = np.full(n, -7, np.int32)
    num_colors, rounds = c_int32(-7), c_int32(-7)
    status = lib().spmv_c_csr_color_cpu(A, _np_ptr(colors), byref(num_colors), byref(rounds),
                                        byref(config) if config is not None else None)
    if status != 0:
        return status, None, 0, 0
    return status, colors, num_colors.value, rounds.value


def color_ordering(n, d_colors, num_colors, d_perm, d_inverse):
    """The vertices sorted by (colour, index) on the device (reorder.h color_ordering): d_perm[new] = old,
    d_inverse[old] = new; returns (status, color_ptr) with color_ptr the num_colors + 1 host offsets."""
    color_ptr = np.full(max(int(num_colors), 0) + 1, -7, np.int32)
    status = lib().spmv_c_color_ordering(int(n), _dev(d_colors), int(num_colors), _dev(d_perm), _dev(d_inverse),
                                         _np_ptr(color_ptr))
    return status, color_ptr


def csr_permute_gpu(B, A, d_row_perm=None, d_col_inverse=None) -> int:
    """B = P A Q^T on the device with sorted rows (reorder.h csr_permute_gpu): row i of B is row d_row_perm[i] of A,
    column j renamed d_col_inverse[j]; None is the identity.  csr_from_gpu(B) fills B's host arrays."""
    return lib().spmv_c_csr_permute_gpu(B, A, _dev(d_row_perm), _dev(d_col_inverse))


def csr_permute_cpu(B, A, row_perm=None, col_inverse=None) -> int:
    """The same on host arrays, the definition of the order (reorder.h csr_permute_cpu); csr_host_arrays(B) reads the
    result."""
    rows = None if row_perm is None else np.ascontiguousarray(row_perm, dtype=np.int32)
    cols = None if col_inverse is None else np.ascontiguousarray(col_inverse, dtype=np.int32)
    return lib().spmv_c_csr_permute_cpu(B, A, None if rows is None else _np_ptr(rows),
                                        None if cols is None else _np_ptr(cols))


def permute_gather(d_out, d_in, d_index, n, k=1, ldo=None, ldi=None) -> int:
    """d_out[i, :k] = d_in[d_index[i], :k] for the rows of an n x k row-major array (reorder.h permute_gather)."""
    k = int(k)
    return lib().spmv_c_permute_gather(_dev(d_out), k if ldo is None else int(ldo), _dev(d_in),
                                       k if ldi is None else int(ldi), _dev(d_index), int(n), k)


def permute_gather_async(d_out, d_in, d_index, n, k=1, ldo=None, ldi=None, stream=None) -> int:
    k = int(k)
    return lib().spmv_c_permute_gather_async(_dev(d_out), k if ldo is None else int(ldo), _dev(d_in),
                                             k if ldi is None else int(ldi), _dev(d_index), int(n), k,
                                             c_void_p(stream))


def multicolor_reorder(B, A, d_perm, d_inverse, config=None) -> ColorResult:
    """Colours A, orders the vertices into d_perm / d_inverse (num_rows int32 each on the device) and forms
    B = P A P^T (reorder.h multicolor_reorder)."""
    out = ColorResult()
    lib().spmv_c_multicolor_reorder(B, A, _dev(d_perm), _dev(d_inverse),
                                    byref(config) if config is not None else None, byref(out))
    return out


# ---- reverse Cuthill-McKee reordering (include/spmv/reorder.h) ---------------------------
def csr_rcm(A, d_perm, d_inverse, config=None) -> RcmResult:
    """The reverse Cuthill-McKee ordering of the square device matrix A into d_perm[new] = old and d_inverse[old] = new
    (num_rows int32 each on the device): the same ints as csr_rcm_cpu (reorder.h csr_rcm)."""
    out = RcmResult()
    lib().spmv_c_csr_rcm(A, _dev(d_perm), _dev(d_inverse), byref(config) if config is not None else None, byref(out))
    return out


def csr_rcm_cpu(A, config=None, perm=None, inverse=None):
    """The ordering on A's host arrays, the definition (reorder.h csr_rcm_cpu): (status, perm, inverse, components,
    levels); perm and inverse are None when the call fails.  perm / inverse: int32 arrays to write into (the tests'
    poisoned ones), allocated here when not given."""
    n = max(A.contents.num_rows, 0) if A else 0
    perm = np.full(n, -7, np.int32) if perm is None else perm
    inverse = np.full(n, -7, np.int32) if inverse is None else inverse
    components, levels = c_int32(-7), c_int32(-7)
    status = lib().spmv_c_csr_rcm_cpu(A, _np_ptr(perm), _np_ptr(inverse), byref(components), byref(levels),
                                      byref(config) if config is not None else None)
    if status != 0:
        return status, None, None, 0, 0
    return status, perm, inverse, components.value, levels.value


def rcm_reorder(B, A, d_perm, d_inverse, config=None) -> RcmResult:
    """csr_rcm, then B = P A P^T on the device (reorder.h rcm_reorder)."""
    out = RcmResult()
    lib().spmv_c_rcm_reorder(B, A, _dev(d_perm), _dev(d_inverse), byref(config) if config is not None else None,
                             byref(out))
    return out


def csr_band_gpu(A):
    """(status, lower, upper, profile) of A's device arrays (reorder.h csr_band_gpu); the figures are None when the
    call fails"""
    out = CsrBand(-7, -7, -7)
    status = lib().spmv_c_csr_band_gpu(A, byref(out))
    return (status, out.lower, out.upper, out.profile) if status == 0 else (status, None, None, None)


def csr_band_cpu(A):
    """the same of A's host arrays (reorder.h csr_band_cpu)"""
    out = CsrBand(-7, -7, -7)
    status = lib().spmv_c_csr_band_cpu(A, byref(out))
    return (status, out.lower, out.upper, out.profile) if status == 0 else (status, None, None, None)


# ---- matrix assembly (include/spmv/assemble.h) ------------------------------------------
COO_SUM, COO_KEEP = 0, 1


def csr_from_coo_cpu(C, num_rows, num_cols, rows, cols, vals, config=None, n=None) -> int:
    """The definition on host arrays (assemble.h csr_from_coo_cpu): C = the matrix of the triplets (rows[p], cols[p],
    vals[p]); csr_host_arrays(C) reads the result.  n defaults to len(rows)."""
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    c = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
    v = None if vals is None else np.ascontiguousarray(vals, dtype=np.float32)
    if n is None:
        n = 0 if r is None else r.size
    return lib().spmv_c_csr_from_coo_cpu(C, int(num_rows), int(num_cols), int(n), None if r is None else _np_ptr(r),
                                         None if c is None else _np_ptr(c), None if v is None else _np_ptr(v),
                                         byref(config) if config is not None else None)


def csr_from_coo_gpu(C, num_rows, num_cols, n, d_rows, d_cols, d_vals, config=None, want_plan=False):
    """C from n device triplets, on the device, bit for bit csr_from_coo_cpu's (assemble.h csr_from_coo_gpu).  Returns
    the CooResult, or (CooResult, plan) with want_plan: the plan (None when the call failed) goes to csr_coo_refill and
    is released with coo_plan_destroy."""
    out = CooResult()
    plan = c_void_p(None)
    lib().spmv_c_csr_from_coo_gpu(C, int(num_rows), int(num_cols), int(n), _dev(d_rows), _dev(d_cols), _dev(d_vals),
                                  byref(config) if config is not None else None,
                                  byref(plan) if want_plan else None, byref(out))
    return (out, plan.value) if want_plan else out


def csr_coo_refill(plan, C, d_vals) -> int:
    """Only C's device values again, from new values in the same triplet order (assemble.h csr_coo_refill)."""
    return lib().spmv_c_csr_coo_refill(c_void_p(plan), C, _dev(d_vals))


def csr_coo_refill_async(plan, C, d_vals, stream=None) -> int:
    return lib().spmv_c_csr_coo_refill_async(c_void_p(plan), C, _dev(d_vals), c_void_p(stream))


def coo_plan_destroy(plan) -> None:
    lib().spmv_c_coo_plan_destroy(c_void_p(plan))


def coo_plan_info(plan):
    """(status, num_rows, num_cols, n, nnz_out, duplicates) of a plan."""
    vals = [c_int32(-7) for _ in range(5)]
    status = lib().spmv_c_coo_plan_info(c_void_p(plan), *[byref(v) for v in vals])
    return (status,) + tuple(v.value for v in vals)


def csr_row_indices_gpu(A, d_rows) -> int:
    """d_rows[p] = the row of stored entry p of the device matrix A (assemble.h csr_row_indices_gpu)."""
    return lib().spmv_c_csr_row_indices_gpu(A, _dev(d_rows))


def csr_add(C, alpha, A, beta, B) -> CsrAddResult:
    """C = alpha*A + beta*B of two device matrices with strictly ascending rows (include/spmv/csr_ops.h csr_add),
    bit-identical to csr_add_cpu; C owns new device arrays afterwards and csr_from_gpu(C) fills its host arrays.
    result.error_code is the return value."""
    out = CsrAddResult()
    out.error_code = lib().spmv_c_csr_add(C, float(alpha), A, float(beta), B, byref(out))
    return out


def csr_add_numeric(C, alpha, A, beta, B) -> CsrAddResult:
    """Only C's device values again, into the pattern an earlier csr_add produced (csr_ops.h csr_add_numeric)."""
    out = CsrAddResult()
    out.error_code = lib().spmv_c_csr_add_numeric(C, float(alpha), A, float(beta), B, byref(out))
    return out


def csr_add_cpu(C, alpha, A, beta, B) -> int:
    """The sum on host arrays, the definition of the arithmetic (csr_ops.h csr_add_cpu); C gets new host arrays."""
    return lib().spmv_c_csr_add_cpu(C, float(alpha), A, float(beta), B)


# ---- block CSR (include/spmv/bsr_matrix.h, include/spmv/bsr.h) -----------------------------------------------
def bsr_create(rows, cols, block_dim, num_blocks):
    p = lib().spmv_c_bsr_create(rows, cols, block_dim, num_blocks)
    return p if p else None


def bsr_destroy(mat) -> None:
    if mat:
        lib().spmv_c_bsr_destroy(mat)


def bsr_to_gpu(mat) -> int:
    return lib().spmv_c_bsr_to_gpu(mat)


def bsr_from_gpu(mat) -> int:
    return lib().spmv_c_bsr_from_gpu(mat)


def bsr_free_gpu(mat) -> None:
    lib().spmv_c_bsr_free_gpu(mat)


def bsr_invalidate_gpu_cache(mat) -> None:
    lib().spmv_c_bsr_invalidate_gpu_cache(mat)


def bsr_wrap_device(rows, cols, block_dim, num_blocks, d_block_row_ptrs, d_block_cols, d_values):
    """Header over caller-owned device arrays (bsr_matrix.h bsr_wrap_device); None for a shape no BSR matrix has."""
    p = lib().spmv_c_bsr_wrap_device(rows, cols, block_dim, num_blocks, c_void_p(d_block_row_ptrs),
                                     c_void_p(d_block_cols), c_void_p(d_values))
    return p if p else None


def bsr_from_arrays(num_rows, num_cols, block_dim, block_row_ptrs, block_cols, values):
    """Convenience: bsr_create + fill of the host arrays."""
    block_row_ptrs = np.ascontiguousarray(block_row_ptrs, dtype=np.int32)
    block_cols = np.ascontiguousarray(block_cols, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    mat = bsr_create(num_rows, num_cols, block_dim, int(block_cols.size))
    m = mat.contents
    assert block_row_ptrs.size == m.num_block_rows + 1 and values.size == block_cols.size * block_dim * block_dim
    ctypes.memmove(m.block_row_ptrs, _np_ptr(block_row_ptrs), block_row_ptrs.nbytes)
    if block_cols.size:
        ctypes.memmove(m.block_cols, _np_ptr(block_cols), block_cols.nbytes)
        ctypes.memmove(m.values, _np_ptr(values), values.nbytes)
    return mat


def bsr_host_arrays(mat):
    """(block_row_ptrs, block_cols, values) numpy copies of the host arrays; values is flat."""
    m = mat.contents
    rp = np.ctypeslib.as_array(m.block_row_ptrs, shape=(m.num_block_rows + 1,)).copy()
    if m.num_blocks > 0:
        bc = np.ctypeslib.as_array(m.block_cols, shape=(m.num_blocks,)).copy()
        va = np.ctypeslib.as_array(m.values, shape=(m.num_blocks * m.block_dim * m.block_dim,)).copy()
    else:
        bc, va = np.empty(0, np.int32), np.empty(0, np.float32)
    return rp, bc, va


def bsr_from_csr_cpu(B, A, block_dim) -> int:
    """CSR (strictly ascending rows) to BSR on host arrays: the definition of the conversion (bsr.h)."""
    return lib().spmv_c_bsr_from_csr_cpu(B, A, int(block_dim))


def bsr_from_csr_gpu(B, A, block_dim) -> BsrBuildResult:
    """The same on the device, bit for bit (bsr.h bsr_from_csr_gpu); B owns new device arrays afterwards and
    bsr_from_gpu(B) fills its host arrays.  result.error_code is the return value."""
    out = BsrBuildResult()
    out.error_code = lib().spmv_c_bsr_from_csr_gpu(B, A, int(block_dim), byref(out))
    return out


def bsr_from_csr_numeric(B, A) -> BsrBuildResult:
    """Only B's device values again from a new A over the same pattern (bsr.h bsr_from_csr_numeric)."""
    out = BsrBuildResult()
    out.error_code = lib().spmv_c_bsr_from_csr_numeric(B, A, byref(out))
    return out


def csr_block_count_gpu(A, block_dim):
    """(status, blocks) of the counting pass alone (bsr.h csr_block_count_gpu)."""
    blocks = c_int64(-1)
    status = lib().spmv_c_csr_block_count_gpu(A, int(block_dim), byref(blocks))
    return status, int(blocks.value)


def bsr_to_csr_gpu(A, B, keep_zeros=0) -> int:
    return lib().spmv_c_bsr_to_csr_gpu(A, B, int(keep_zeros))


def bsr_to_csr_cpu(A, B, keep_zeros=0) -> int:
    return lib().spmv_c_bsr_to_csr_cpu(A, B, int(keep_zeros))


def spmv_cpu_bsr(A, x) -> np.ndarray:
    """The ordered sum on host arrays (bsr.h spmv_cpu_bsr)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.zeros(A.contents.num_rows, dtype=np.float32)
    lib().spmv_c_cpu_bsr(A, _np_ptr(x), _np_ptr(y))
    return y


def spmv_bsr(A, d_x, d_y, config=None, vec_size=-1) -> SpMVResult:
    out = SpMVResult()
    out.error_code = lib().spmv_c_spmv_bsr(A, _dev(d_x), _dev(d_y), byref(config) if config is not None else None,
                                           vec_size, byref(out))
    return out


def spmv_bsr_async(A, d_x, d_y, config=None, vec_size=-1, stream=None) -> int:
    return lib().spmv_c_spmv_bsr_async(A, _dev(d_x), _dev(d_y), byref(config) if config is not None else None,
                                       vec_size, c_void_p(stream))


def compute_bandwidth_bsr(A, elapsed_ms) -> BandwidthMetrics:
    out = BandwidthMetrics()
    lib().spmv_c_compute_bandwidth_bsr(A, float(elapsed_ms), byref(out))
    return out


def bsr_diag_inverse_cpu(A):
    """(status, inv): the fp32 inverses of A's diagonal blocks on host arrays, num_block_rows * b * b floats (bsr.h
    bsr_diag_inverse_cpu: the definition of the block-Jacobi factor)."""
    c = A.contents
    count = c.num_block_rows * c.block_dim * c.block_dim
    inv = np.zeros(max(count, 1), np.float32)
    status = lib().spmv_c_bsr_diag_inverse_cpu(A, _np_ptr(inv))
    return status, inv[:count]


def bsr_diag_inverse_gpu(A, d_inv) -> int:
    """The same bits into a device array (bsr.h bsr_diag_inverse_gpu)."""
    return lib().spmv_c_bsr_diag_inverse_gpu(A, _dev(d_inv))


def bsr_diag_apply_cpu(A, inv, r) -> np.ndarray:
    """z = D^-1 r by the ordered sum on host arrays (bsr.h bsr_diag_apply_cpu)."""
    inv = np.ascontiguousarray(inv, np.float32)
    r = np.ascontiguousarray(r, np.float32)
    z = np.zeros(max(A.contents.num_rows, 1), np.float32)
    lib().spmv_c_bsr_diag_apply_cpu(A, _np_ptr(inv), _np_ptr(r), _np_ptr(z))
    return z[:A.contents.num_rows]


def bsr_diag_apply(A, d_inv, d_r, d_z) -> int:
    """The same on device arrays (bsr.h bsr_diag_apply)."""
    return lib().spmv_c_bsr_diag_apply(A, _dev(d_inv), _dev(d_r), _dev(d_z))


def cg_solve_bsr(A, d_b, d_x, config=None) -> CGResult:
    """CG on a BSR matrix with preconditioner 0 NONE, 1 JACOBI or 2 BLOCK_JACOBI (include/spmv/cg.h cg_solve_bsr)."""
    out = CGResult()
    lib().spmv_c_cg_solve_bsr(A, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


# ---- block IC(0) and the block triangular solves (include/spmv/bsr_factor.h) ---------------------------------
def bsr_ic0_cpu(A):
    """Block IC(0) on A's host arrays (bsr_factor.h bsr_ic0_cpu, the definition of the arithmetic): returns
    (f_values, bad_pivot), f_values in the factor format of bsr_factor.h; raises ValueError with the library's error
    string when the call is rejected."""
    c = A.contents
    f = np.zeros(max(c.num_blocks * c.block_dim * c.block_dim, 1), np.float32)
    pivot = c_int32(-1)
    status = lib().spmv_c_bsr_ic0_cpu(A, _np_ptr(f), byref(pivot))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return f[:c.num_blocks * c.block_dim * c.block_dim], pivot.value


def bsr_ic0(A, d_f_values) -> IC0Result:
    """Block IC(0) of the square device BSR matrix A into d_f_values, num_blocks * b * b floats in A's block pattern
    (bsr_factor.h bsr_ic0; may be A's own device values: in place).  lanes_per_row and bad_pivot count BLOCK rows.
    bsr_wrap_device over A's structure arrays and d_f_values is the factor matrix of sptrsv_bsr and cg_solve_bsr_ic."""
    out = IC0Result()
    lib().spmv_c_bsr_ic0(A, _dev(d_f_values), byref(out))
    return out


def bsr_ic0_async(A, d_f_values, stream=None) -> int:
    return lib().spmv_c_bsr_ic0_async(A, _dev(d_f_values), c_void_p(stream))


def sptrsv_cpu_bsr(F, b, x=None, config=None):
    """(status, x): T x = b on host arrays, T the config.uplo block triangle of F in the factor format (bsr_factor.h
    sptrsv_cpu_bsr, the definition of the ordered solve).  x: the array solved into (b itself solves in place)."""
    b = np.ascontiguousarray(b, np.float32) if x is not b else b
    if x is None:
        x = np.zeros(max(F.contents.num_rows, 1), np.float32)
    status = lib().spmv_c_sptrsv_cpu_bsr(F, _np_ptr(b), _np_ptr(x), byref(config) if config is not None else None)
    return status, x[:F.contents.num_rows]


def sptrsv_bsr(F, d_b, d_x, config=None) -> SpTRSVResult:
    """The block triangular solve on the device (bsr_factor.h sptrsv_bsr); d_b may be d_x (in place)."""
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_bsr(F, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def sptrsv_bsr_async(F, d_b, d_x, config=None, stream=None) -> int:
    return lib().spmv_c_sptrsv_bsr_async(F, _dev(d_b), _dev(d_x), byref(config) if config is not None else None,
                                         c_void_p(stream))


def sptrsv_analyze_bsr(A, uplo=0) -> SpTRSVResult:
    """Builds and caches the level schedule of the `uplo` triangle of A's block pattern ahead of a timed call."""
    out = SpTRSVResult()
    lib().spmv_c_sptrsv_analyze_bsr(A, int(uplo), byref(out))
    return out


def cg_solve_bsr_ic(A, F, d_b, d_x, config=None) -> CGResult:
    """CG on a BSR matrix preconditioned with the block IC(0) factor matrix F (include/spmv/cg.h cg_solve_bsr_ic)."""
    out = CGResult()
    lib().spmv_c_cg_solve_bsr_ic(A, F, _dev(d_b), _dev(d_x), byref(config) if config is not None else None, byref(out))
    return out


def csr_scale_gpu(A, d_row_scale=None, d_col_scale=None, d_values_out=None) -> int:
    """out[p] = a[p] * (r[row] * c[col]) on the device (csr_ops.h csr_scale_gpu); a scale may be None; d_values_out
    None = in place into A's device values."""
    return lib().spmv_c_csr_scale_gpu(A, _dev(d_row_scale), _dev(d_col_scale), _dev(d_values_out))


def _f32_or_none(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def csr_scale_cpu(A, row_scale=None, col_scale=None):
    """(status, values) of the same scaling of A's host arrays (csr_ops.h csr_scale_cpu)."""
    r, c = _f32_or_none(row_scale), _f32_or_none(col_scale)
    out = np.empty(max(int(A.contents.nnz), 0), np.float32)
    status = lib().spmv_c_csr_scale_cpu(A, None if r is None else _np_ptr(r), None if c is None else _np_ptr(c),
                                        _np_ptr(out))
    return status, out


def csr_diagonal_gpu(A, d_diag) -> int:
    """d_diag[i] = the fp32 sum of row i's stored (i, i) entries, 0 where there is none (csr_ops.h csr_diagonal_gpu)."""
    return lib().spmv_c_csr_diagonal_gpu(A, _dev(d_diag))


def csr_diagonal_cpu(A):
    """(status, diag) of the same on A's host arrays (csr_ops.h csr_diagonal_cpu)."""
    out = np.empty(max(int(A.contents.num_rows), 0), np.float32)
    status = lib().spmv_c_csr_diagonal_cpu(A, _np_ptr(out))
    return status, out


def csr_diag_matrix_gpu(D, n, d_diag=None) -> int:
    """D = the n x n diagonal matrix of the device vector d_diag, the identity when it is None (csr_ops.h
    csr_diag_matrix_gpu); D owns new device arrays afterwards."""
    return lib().spmv_c_csr_diag_matrix_gpu(D, int(n), _dev(d_diag))


def csr_diag_matrix_cpu(D, n, diag=None) -> int:
    """The same on the host: D gets new host arrays (csr_ops.h csr_diag_matrix_cpu)."""
    d = _f32_or_none(diag)
    assert d is None or d.size >= n
    return lib().spmv_c_csr_diag_matrix_cpu(D, int(n), None if d is None else _np_ptr(d))


def spmv_auto_config(A) -> SpMVConfig:
    out = SpMVConfig()
    status = lib().spmv_c_auto_config(A, byref(out))
    if status != 0:
        raise ValueError(spmv_error_string(status))
    return out


def spmv_validate_dimensions(num_cols, vec_size) -> bool:
    return bool(lib().spmv_c_validate_dimensions(num_cols, vec_size))


# ---- bandwidth (reference include/spmv/bandwidth.h:21-27) ---------------------------
def compute_bandwidth_csr(A, elapsed_ms) -> BandwidthMetrics:
    out = BandwidthMetrics()
    lib().spmv_c_compute_bandwidth_csr(A, elapsed_ms, byref(out))
    return out


def compute_bandwidth_ell(A, elapsed_ms) -> BandwidthMetrics:
    out = BandwidthMetrics()
    lib().spmv_c_compute_bandwidth_ell(A, elapsed_ms, byref(out))
    return out


def compute_bandwidth_csr_multi(A, k, elapsed_ms) -> BandwidthMetrics:
    """Byte model of spmv_csr_multi: nnz*8 + (rows+1)*4 + k*cols*4 + k*rows*4."""
    out = BandwidthMetrics()
    lib().spmv_c_compute_bandwidth_csr_multi(A, int(k), elapsed_ms, byref(out))
    return out


def get_gpu_peak_bandwidth() -> float:
    return float(lib().spmv_c_get_gpu_peak_bandwidth())


# ---- PageRank (reference include/spmv/pagerank.h:29-43) -----------------------------
def pagerank(adj_matrix, config=None) -> PageRankResult:
    raw = _PageRankResultC()
    lib().spmv_c_pagerank(adj_matrix, byref(config) if config is not None else None, byref(raw))
    if not raw.ranks:
        return PageRankResult(None, 0, 0.0, False)
    n = adj_matrix.contents.num_rows
    if n < (1 << 18):
        ranks = np.ctypeslib.as_array(raw.ranks, shape=(n,)).copy() if n > 0 else np.empty(0, np.float32)
        lib().spmv_c_pagerank_free(byref(raw))
    else:
        # large result: a view of the library's (pinned, pooled) array, handed back by pagerank_free when the
        # numpy array is collected — no 4n-byte host copy
        ranks = np.ctypeslib.as_array(raw.ranks, shape=(n,))
        import weakref
        weakref.finalize(ranks, lambda held=raw: lib().spmv_c_pagerank_free(byref(held)))
    return PageRankResult(ranks, raw.iterations, float(raw.final_residual), bool(raw.converged))


def pagerank_multi_gpu(adj_matrix, config=None, num_gpus=1) -> PageRankResult:
    """include/spmv/pagerank.h extension: the row-sharded single-process RCCL loop over `num_gpus` devices."""
    raw = _PageRankResultC()
    lib().spmv_c_pagerank_multi_gpu(adj_matrix, byref(config) if config is not None else None, num_gpus, byref(raw))
    if not raw.ranks:
        return PageRankResult(None, 0, 0.0, False)
    n = adj_matrix.contents.num_rows
    ranks = np.ctypeslib.as_array(raw.ranks, shape=(n,)).copy()
    lib().spmv_c_pagerank_free(byref(raw))
    return PageRankResult(ranks, raw.iterations, float(raw.final_residual), bool(raw.converged))


def pagerank_personalized(adj_matrix, d_V, d_R, k, ldv=None, ldr=None, config=None) -> list:
    """Personalized PageRank for k teleport vectors in one matrix pass per step (include/spmv/pagerank.h
    pagerank_personalized): d_V (read only) and d_R are num_rows x k row-major device arrays with leading dimensions
    ldv, ldr >= k (default k); returns one PersonalizedResult per column (at least one, so that a rejected call always
    has somewhere to report its error_code)."""
    k = int(k)
    ldv = k if ldv is None else int(ldv)
    ldr = k if ldr is None else int(ldr)
    out = (PersonalizedResult * max(k, 1))()
    rc = lib().spmv_c_pagerank_personalized(adj_matrix, _dev(d_V), ldv, _dev(d_R), ldr, k,
                                            byref(config) if config is not None else None, out)
    results = list(out)
    if rc != 0:
        for r in results:
            r.error_code = rc
    return results


def pagerank_personalized_seeds(adj_matrix, seed_sets, d_R, ldr=None, config=None) -> list:
    """pagerank_personalized with column j teleporting uniformly to the nodes of seed_sets[j] (a sequence of k
    sequences of node ids); one PersonalizedResult per set."""
    k = len(seed_sets)
    ldr = k if ldr is None else int(ldr)
    ptrs = np.zeros(k + 1, np.int32)
    ptrs[1:] = np.cumsum([len(s) for s in seed_sets], dtype=np.int64)
    # (one spare entry: never an empty array)
    nodes = np.concatenate([np.asarray(s, np.int64).ravel() for s in seed_sets] + [np.zeros(1, np.int64)]).astype(np.int32)
    out = (PersonalizedResult * max(k, 1))()
    rc = lib().spmv_c_pagerank_personalized_seeds(adj_matrix, _np_ptr(ptrs), _np_ptr(nodes), k, _dev(d_R), ldr,
                                                  byref(config) if config is not None else None, out)
    results = list(out)
    if rc != 0:
        for r in results:
            r.error_code = rc
    return results


def pagerank_top_k(result: PageRankResult, num_nodes: int, k: int):
    """[(node_id, rank)] of the k best-ranked nodes, descending."""
    if result is None or result.ranks is None or k <= 0 or num_nodes <= 0:
        return []
    ranks = np.ascontiguousarray(result.ranks, dtype=np.float32)
    raw = _PageRankResultC()
    raw.ranks = ranks.ctypes.data_as(POINTER(c_float))
    keep = min(k, num_nodes)
    nodes = (TopKNode * keep)()
    lib().spmv_c_pagerank_top_k(byref(raw), num_nodes, k, nodes)
    return [(n.node_id, float(n.rank)) for n in nodes]


from . import synth  # noqa: E402,F401  (numpy twin of the device generators)
