// spmv/bsr.h — block CSR (BSR): conversion from and to CSR on the device and on the host, bit for bit the same, a
// values-only refill, and y = A x on a BSRMatrix (kernels in gpu-spmv_amd/csrc/bsr.hip, host twins and argument checks
// in bsr_host.cpp; when to convert is in INTEGRATION.md), and the inverses of the diagonal blocks
// with their apply, the block-Jacobi preconditioner of cg_solve_bsr (cg_bsr.hip, bsr_diag_host.cpp).
//
// Everything is fp32 values and int32 indices; the container and its layout are in spmv/bsr_matrix.h.
//
// The conversion (bsr_from_csr_cpu is its definition): A's columns must be STRICTLY ASCENDING inside every row
// (csr_add's rule).  Block row I holds one block for every block column J that any of A's rows I*b .. I*b+b-1 touches,
// J ascending.  Every stored entry of A is copied bit for bit into its position (-0.0f, NaN payloads, denormals and
// explicit zeros included); every other position is +0.0f.
//
// The product (spmv_cpu_bsr is the definition of the ordered sum): for scalar row i = I*b + r < num_rows,
//     s = +0.0f;  over the blocks of block row I in stored order, over c = 0 .. b-1 with J*b + c < num_cols:
//     s = fl(s + fl(v * x[J*b + c]))
// multiply and add rounded separately, as spmv_cpu_csr does.  Positions outside the matrix are SKIPPED, not
// multiplied: x is never read at or past num_cols and y is never written at or past num_rows.  The padding zeros
// INSIDE the matrix are real entries: 0 * Inf = NaN, as IEEE says, so a matrix with padding answers an x that holds
// Inf or NaN differently from its CSR source.  For finite x and a BSR matrix converted from a CSR matrix with sorted
// rows the ordered result equals spmv_cpu_csr on that CSR matrix bit for bit: the inserted products are +-0 and a
// running sum that starts at +0.0f is never -0.0f.
#ifndef SPMV_BSR_H
#define SPMV_BSR_H

#include "bandwidth.h"
#include "bsr_matrix.h"
#include "common.h"
#include "csr_matrix.h"
#include "spmv.h"

namespace spmv {

struct BsrBuildResult {
    int   error_code;      // SpMVError as int
    int   num_blocks;      // blocks of B
    float fill;            // nnz / (positions of all blocks that lie inside the matrix), computed in double; 0 without blocks
    int   max_block_row;   // most blocks in one block row
    int   lanes;           // lanes that share one block row
    int   launches;        // kernel launches of the call
    float symbolic_ms;     // device-event time of the counting pass and the scan (0 for bsr_from_csr_numeric)
    float numeric_ms;      // device-event time of the fill
    BsrBuildResult() : error_code(0), num_blocks(0), fill(0.0f), max_block_row(0), lanes(0), launches(0),
                       symbolic_ms(0.0f), numeric_ms(0.0f) {}
};

// The conversion on HOST arrays, by the rule above.
// Checks, in this order, B untouched when one fails: null B / A -> INVALID_ARGUMENT; unsupported block_dim ->
// INVALID_ARGUMENT; missing host arrays, row pointers that do not start at 0, decrease or do not end at nnz, a column
// outside [0, n) or not strictly above its left neighbour -> INVALID_FORMAT; more than INT_MAX blocks ->
// INVALID_DIMENSION.  On SUCCESS B gets new host arrays (owns_host_memory); its device arrays, which would be stale,
// are freed.
int bsr_from_csr_cpu(BSRMatrix* B, const CSRMatrix* A, int block_dim);

// The conversion of a device-resident A (csr_to_gpu / csr_wrap_device; the arrays may be views at any 4-byte offset):
// the same ints and the same bits as bsr_from_csr_cpu on every run, stream and lane count.  B is handed over as
// csr_add hands over C: it owns new device arrays, its host arrays are allocated at the new size and hold no data
// until bsr_from_gpu(B); what B owned before is released.  Runs on the library stream (spmv_set_stream) and returns
// after completion, all scratch (4 B per entry of A) freed.
//
// A counting pass, an exclusive scan, a fill; no sort, no float atomics, no workgroup waits for another.  A group of
// `lanes` lanes owns a block row and strides over the entries of its b rows, which are contiguous in A.  An entry
// OWNS its block when it is the first of its row with that block column and no earlier row of the block row touches
// the block column (a binary search per earlier row).  The counting pass counts the owners, and leaves for every
// entry the number of owners before it in the block row.  After the scan the rank of block column J in its block row
// is the number of owners left of J, summed over the b rows from those prefixes: owners write their block column at
// that rank, and every entry then finds its block by a search in the finished block row and writes its value.  One
// writer per slot, nothing depends on the lane count.
//
// Checks, in this order, B untouched by every failure:
//   1. null B / A -> INVALID_ARGUMENT
//   2. unsupported block_dim -> INVALID_ARGUMENT
//   3. missing device arrays (the rule of csr_transpose_gpu) -> INVALID_FORMAT
//   4. on the device, before B is allocated: row pointers start at 0, do not decrease and end at nnz; every column
//      in [0, n) and strictly above its left neighbour -> INVALID_FORMAT
//   5. more than INT_MAX blocks -> INVALID_DIMENSION
//   6. allocation failure -> CUDA_MALLOC, nothing leaked
// m == 0, n == 0 or nnz == 0 give a valid B with no blocks.
// result (may be null) receives the statistics; the return value equals result->error_code.
int bsr_from_csr_gpu(BSRMatrix* B, const CSRMatrix* A, int block_dim, BsrBuildResult* result = nullptr);

// Refills only B->d_values from a new A over the same pattern (new values after csr_coo_refill, a time-stepping
// loop): the values are zeroed and scattered, no allocation beyond a flag word.  The pass checks A while it runs (row
// pointers, columns in range) and that every entry of A finds its block; a block that no entry touches any more stays
// stored, all zero.  Checks: 1 and 3 as above, then B must be m×n (INVALID_DIMENSION) and have device arrays
// (INVALID_FORMAT); an entry of A whose block is not in B (or a malformed A) -> INVALID_FORMAT, with B's values
// unspecified.  B's structure arrays are never written.  Ends with bsr_invalidate_gpu_cache(B).  result receives
// num_blocks (B's), lanes, launches (1) and numeric_ms.
int bsr_from_csr_numeric(BSRMatrix* B, const CSRMatrix* A, BsrBuildResult* result = nullptr);

// The counting pass alone: *blocks = the blocks bsr_from_csr_gpu(A, block_dim) would store, so that a caller can
// compute the fill nnz / (blocks * b * b) and decide before paying for the build (BSR moves fewer
// matrix bytes than CSR when fill > 1/2 + 1/(2 b^2)).  Checks 1 - 4 as above (null blocks -> INVALID_ARGUMENT).
int csr_block_count_gpu(const CSRMatrix* A, int block_dim, long long* blocks);

// BSR back to CSR with sorted rows.  keep_zeros != 0: every position of every block that lies inside the matrix;
// keep_zeros == 0: the positions whose value is not +-0.0f (NaN is kept), so CSR -> BSR -> CSR returns a matrix
// without stored zeros bit for bit.  A counting pass, a scan, a fill; A is handed over as csr_add hands over C
// (bsr_to_csr_cpu: new host arrays).
// Checks, in this order, A untouched by every failure: null A / B -> INVALID_ARGUMENT; a bad shape (block_dim,
// negative sizes, block counts that do not match the scalar sizes) or missing arrays -> INVALID_FORMAT; block row
// pointers by the CSR rule, block columns in [0, num_block_cols) and strictly ascending (on the device first, before
// anything is allocated for A) -> INVALID_FORMAT; more than INT_MAX entries -> INVALID_DIMENSION; allocation failure ->
// CUDA_MALLOC.
int bsr_to_csr_gpu(CSRMatrix* A, const BSRMatrix* B, int keep_zeros);
int bsr_to_csr_cpu(CSRMatrix* A, const BSRMatrix* B, int keep_zeros);

// Host path: the definition of the ordered sum (above).  Nothing is checked, as in spmv_cpu_csr.
void spmv_cpu_bsr(const BSRMatrix* A, const float* x, float* y);

// Device path.  config->kernel_type selects
//   SCALAR_CSR, ELL_KERNEL, or config == nullptr   the CPU-order kernel: one lane per scalar row, bit-identical to
//                                                  spmv_cpu_bsr (no FMA contraction)
//   VECTOR_CSR, MERGE_PATH                         the lane-group kernel (there is no merge-path form for blocks:
//                                                  MERGE_PATH names the same kernel): an aligned group of 1 .. 64 lanes
//                                                  owns a block row, each lane holds b accumulators and takes whole
//                                                  blocks; deterministic at a fixed lane count, which is
//                                                  pick_lanes_per_row of TWICE the mean blocks per block row (the
//                                                  smallest group with 2 * lanes >= the mean: two steps a block row,
//                                                  the measured variant; SPMV_DEBUG=bsr_lanes=N forces one)
// use_texture is accepted and ignored.
// Checks, order and codes as spmv_csr: null A / d_x / d_y -> INVALID_ARGUMENT; num_rows == 0 -> SUCCESS, nothing
// written; vec_size >= 0 and != num_cols -> INVALID_DIMENSION; missing device arrays -> INVALID_FORMAT; block_size
// outside 1 .. 1024 -> KERNEL_LAUNCH.  num_blocks == 0 writes zeros to y[0, num_rows).
// gflops counts STORED flops, 2 * num_blocks * b * b / time: padding is work the kernel does, not useful work.
SpMVResult spmv_bsr(const BSRMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config, int vec_size = -1);
int        spmv_bsr_async(const BSRMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config, int vec_size,
                          hipStream_t stream);

// (the byte model of the GB/s figure is compute_bandwidth_bsr in spmv/bandwidth.h)

// ---- the diagonal blocks: block-Jacobi (the solver that uses them is cg_solve_bsr in spmv/cg.h) ----
// inv (num_block_rows * b * b floats; block I row-major) = fl32(D_I^-1), D_I the stored block (I, I) of a square A, of
// which only the lower triangle (r >= c) is read.  bsr_diag_inverse_cpu (host arrays) is the definition, in fp64 with
// every product, sum, division and root rounded on its own (no fused multiply-add):
//   Cholesky D = L L^T row by row: w = d_pq - sum_{k<q} l_pk l_qk, k ascending, each product subtracted in turn;
//       l_pp = sqrt(w), l_pq = w / l_qq
//   W = L^-1 by forward substitution: w_jj = 1 / l_jj; w_ij = -(sum_{k=j..i-1} l_ik w_kj) / l_ii, k ascending from +0
//   D^-1_ij = sum_{k >= max(i,j)} w_ki w_kj, k ascending from +0, then ONE rounding to fp32; computed for i >= j and
//       stored at (i,j) and (j,i): the result is symmetric bit for bit
// When num_rows is no multiple of b the last block is its leading (num_rows - I*b)-square part; the other rows and
// columns of its inverse are +0.0f.
// Checks, in this order: null A / inv -> INVALID_ARGUMENT; A not square -> INVALID_DIMENSION; a bad shape or missing
// arrays (host arrays for _cpu, device arrays for _gpu) -> INVALID_FORMAT; a block row without a stored diagonal block,
// or a pivot w that is not > 0 or not finite -> INVALID_ARGUMENT, with inv unspecified.  Block columns must be strictly
// ascending inside a block row (the container's rule): the diagonal block is found by a binary search.
int bsr_diag_inverse_cpu(const BSRMatrix* A, float* inv);
// The same bits on the device on every run: one launch, one lane per block row, the block in registers.  d_inv is a
// device array (any 4-byte offset).  The last check is made on the device, in one flag word and one read-back.  Runs
// on the library stream and returns after completion.
int bsr_diag_inverse_gpu(const BSRMatrix* A, float* d_inv);

// z = D^-1 r block by block.  bsr_diag_apply_cpu is the definition of the ordered sum: for row i = I*b + k,
//     s = +0.0f;  for c = 0 .. b-1 with I*b + c < num_rows:  s = fl(s + fl(inv[I][k][c] * r[I*b + c]))
// multiply and add rounded separately.  Only A's shape is read.  Nothing is checked on the host path.
void bsr_diag_apply_cpu(const BSRMatrix* A, const float* inv, const float* r, float* z);
// The device path, bit for bit the same: one thread per scalar row, d_r and d_z distinct arrays of num_rows floats.
// Checks: null A / d_inv / d_r / d_z -> INVALID_ARGUMENT; A not square -> INVALID_DIMENSION; a bad shape ->
// INVALID_FORMAT.  Runs on the library stream and returns after completion.
int  bsr_diag_apply(const BSRMatrix* A, const float* d_inv, const float* d_r, float* d_z);

} // namespace spmv

#endif // SPMV_BSR_H
