// spmv/spmv.h — the SpMV entry points (y = A * x, fp32, int32 indices).
//
// Signatures, struct layouts and defaults follow the reference
// (include/spmv/spmv.h:11-54): SpMVConfig is 12 bytes defaulting to
// {SCALAR_CSR, 256, false}; SpMVResult is 24 bytes returned by value.
// The kernels behind spmv_csr / spmv_ell are hand-written HIP for gfx950
// (gpu-spmv_amd/csrc/); see DESIGN.md for what each KernelType launches.
#ifndef SPMV_SPMV_H
#define SPMV_SPMV_H

#include "common.h"
#include "csr_matrix.h"
#include "ell_matrix.h"

namespace spmv {

struct SpMVConfig {
    enum KernelType {
        SCALAR_CSR,   // per-row sequential sum (CPU summation order, bit-exact)
        VECTOR_CSR,   // a sub-wavefront lane group (2..64 lanes) per row, DPP reduction
        MERGE_PATH,   // equal (rows + nnz) shares per workgroup, deterministic fix-up
        ELL_KERNEL    // ELL only; passed to spmv_csr it behaves as SCALAR_CSR
    };

    KernelType kernel_type;
    int  block_size;    // threads per workgroup; multiple of 64 is used on gfx950
    bool use_texture;   // hint: keep x on chip (LDS tile / L2-resident); no texture unit on CDNA4

    SpMVConfig() : kernel_type(SCALAR_CSR), block_size(256), use_texture(false) {}
};

struct SpMVResult {
    float* y;               // aliases the caller's d_y
    float  elapsed_ms;      // device-event time of the launch(es)
    float  gflops;          // 2 * nnz / time
    float  bandwidth_gb_s;  // algorithmic bytes / time (bandwidth.h)
    int    error_code;      // SpMVError as int, 0 = success

    SpMVResult() : y(nullptr), elapsed_ms(0.0f), gflops(0.0f),
                   bandwidth_gb_s(0.0f), error_code(0) {}
};

// Host reference path (sequential fp32), kept for API parity with the reference.
void spmv_cpu_csr(const CSRMatrix* A, const float* x, float* y);
void spmv_cpu_ell(const ELLMatrix* A, const float* x, float* y);

// Device path.  d_x / d_y are device pointers; vec_size < 0 skips the
// num_cols == vec_size check.  Synchronous: returns after the kernel finished.
SpMVResult spmv_csr(const CSRMatrix* A, const float* d_x, float* d_y,
                    const SpMVConfig* config, int vec_size = -1);
SpMVResult spmv_ell(const ELLMatrix* A, const float* d_x, float* d_y,
                    const SpMVConfig* config, int vec_size = -1);

// Picks a kernel from the row-length statistics (thresholds tuned for wave64).
SpMVConfig spmv_auto_config(const CSRMatrix* A);

inline bool spmv_validate_dimensions(int num_cols, int vec_size) {
    return num_cols == vec_size;
}

// ---- extensions beyond the reference surface (do not change any layout) ----

// Enqueue-only variant: validates, launches on `stream`, does not time or
// synchronise.  Returns an SpMVError as int.  Safe inside hipGraph capture.
// Calls on one matrix from different streams may run at once, as with the reference's stateless kernels: what
// a call writes next to the matrix (the tiled plan's product stream, merge-path's carry-out slots) exists once
// per stream, allocated at a stream's first call on that matrix (also inside a graph capture); beyond eight
// streams per matrix the tiled engine steps aside for the direct kernels.  The first call that BUILDS a
// matrix's auxiliary data allocates and synchronises its stream — do that one outside a capture.
int spmv_csr_async(const CSRMatrix* A, const float* d_x, float* d_y,
                   const SpMVConfig* config, int vec_size, hipStream_t stream);
int spmv_ell_async(const ELLMatrix* A, const float* d_x, float* d_y,
                   const SpMVConfig* config, int vec_size, hipStream_t stream);

// Multi-vector SpMV (csrmm / SpMM): Y = A * X for k right-hand sides in one pass over the matrix.
// Y[i*ldy + j] = sum_p A(i,p) * X[p*ldx + j] for 0 <= i < num_rows, 0 <= j < k.
// X is num_cols x k, Y is num_rows x k, both row-major with leading dimensions ldx, ldy >= k (device pointers).
// Y's columns k..ldy-1 are never written.  Offsets into X and Y are 64-bit (num_cols*ldx, num_rows*ldy may
// exceed 2^31).  Checks, in this order: null A / d_X / d_Y -> INVALID_ARGUMENT; num_rows == 0 -> SUCCESS, nothing
// written; k < 1 -> INVALID_ARGUMENT; vec_size >= 0 && vec_size != num_cols -> INVALID_DIMENSION; ldx < k or ldy < k
// -> INVALID_DIMENSION; missing device arrays -> INVALID_FORMAT; the used ranges of X and Y overlap ->
// INVALID_ARGUMENT; a bad block_size -> as spmv_csr.  nnz == 0 writes zeros to Y[i, 0:k].
// Kernels: SCALAR_CSR (also config == nullptr and ELL_KERNEL) gives columns bit-identical to spmv_cpu_csr(A, X[:, j]);
// VECTOR_CSR and MERGE_PATH may reorder a row's sum.  Every kernel type is bitwise reproducible from run to run.
// use_texture is accepted and ignored: multi calls never build or use the LDS-tiled plan and never count toward
// promotion.  elapsed_ms is device-event time, gflops = 2*nnz*k / time, bandwidth_gb_s from
// compute_bandwidth_csr_multi; one-time preparation (MERGE_PATH's partition and carry slots) happens before the
// start event.  The async variant follows spmv_csr_async's stream rules; a MERGE_PATH call that needs more carry
// columns than its stream holds synchronises that stream once to grow them — do that one outside a graph capture.
SpMVResult spmv_csr_multi(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                          const SpMVConfig* config, int vec_size = -1);
int spmv_csr_multi_async(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                         const SpMVConfig* config, int vec_size, hipStream_t stream);

// Transposed SpMV: y = A^T * x, i.e. y[c] = sum_r A(r,c) * x[r]; d_x holds num_rows entries, d_y num_cols.
// The first call on a matrix builds its device transpose (csr_transpose_gpu's result, before the start event) and
// keeps it with the matrix, next to the other per-matrix data; every call then runs spmv_csr's kernels on it with the
// caller's config (SCALAR_CSR / nullptr / ELL_KERNEL: CPU order, bit-identical to spmv_cpu_csr on the host
// transpose, i.e. to the fp32 loop y[col[p]] += val[p] * x[row(p)] in p order; VECTOR_CSR, MERGE_PATH and
// use_texture as spmv_csr on the transpose).  Every kernel type gives exactly the bits of
// spmv_csr(csr_transpose_gpu(A), ...) with the same config.  Promotion counts on the transpose, never on A; a
// transpose call leaves A's own plan, merge-path state and promotion count alone.
// Checks, in this order: null A / d_x / d_y -> INVALID_ARGUMENT; num_cols == 0 -> SUCCESS, nothing written;
// vec_size >= 0 && vec_size != num_rows -> INVALID_DIMENSION; missing device arrays -> INVALID_FORMAT; a bad
// block_size -> as spmv_csr; then the build's own errors (csr_transpose_gpu).  num_rows == 0 or nnz == 0 writes
// zeros to y[0:num_cols].  elapsed_ms times the SpMV only; gflops = 2*nnz / time; bandwidth_gb_s is
// compute_bandwidth_csr of the transpose.  The cached transpose is a COPY: after writing into A's device arrays in
// place call csr_invalidate_gpu_cache(A) (the same rule as for the tiled plan); swapped arrays, a re-upload and
// csr_free_gpu are noticed on their own.  The async variant follows spmv_csr_async's rules; the call that builds
// the transpose synchronises its stream — make that one outside a graph capture.
SpMVResult spmv_csr_transpose(const CSRMatrix* A, const float* d_x, float* d_y,
                              const SpMVConfig* config, int vec_size = -1);
int spmv_csr_transpose_async(const CSRMatrix* A, const float* d_x, float* d_y,
                             const SpMVConfig* config, int vec_size, hipStream_t stream);

// Promotion of callers that spell a reordering kernel without use_texture (the reference's own callers do:
// benchmarks/main.cu:52-56, src/pagerank.cu:89-90): after `calls` spmv_csr() calls with VECTOR_CSR / MERGE_PATH on a
// matrix the LDS-tiled engine would take (> 32768 columns, >= 1 M entries), the next call builds the matrix's plan in
// front of its timed region and all later ones run on the engine — ~5x faster on a 10 M-row matrix; results stay within
// the 1e-5 bound on both sides of the switch but low-order bits may change there.  Default 4; 0 = never promote
// (environment: SPMV_TILED_PROMOTE=0).  SCALAR_CSR and spmv_ell keep their CPU-order kernels regardless.
void spmv_set_tiled_promotion(int calls);
int spmv_get_tiled_promotion();

// Stream used by the synchronous entry points (default: the null stream).
void spmv_set_stream(hipStream_t stream);
hipStream_t spmv_get_stream();

} // namespace spmv

#endif // SPMV_SPMV_H
