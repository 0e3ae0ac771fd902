// spmv/assemble.h — matrix assembly on the device: a CSR matrix from unsorted (row, column, value) triplets with
// repeats, a plan that refills its values from a new value array in one launch, and the inverse expansion of a CSR
// matrix into the row of every stored entry.
//
// Why: finite-element and finite-volume codes emit contributions element by element, unsorted, with every shared node
// repeated; graph codes emit edge lists.  Everything downstream (sptrsv_analyze_device, ic0_csr, amg_setup_device, the
// solvers) takes a device-resident CSR matrix, and nothing could make one on the device.  Nonlinear and time-stepping
// callers reassemble at every step although only the values changed: csr_coo_refill writes the new values into the
// pattern of the first assembly, upstream of amg_update and spgemm_csr_numeric
// (gpu-spmv_amd/csrc/assemble.hip, assemble_host.cpp; the recipe is in INTEGRATION.md).
#ifndef SPMV_ASSEMBLE_H
#define SPMV_ASSEMBLE_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

enum CooDuplicates {
    COO_SUM  = 0,   // every run of equal (row, column) becomes one entry: the sum of its values in source order
    COO_KEEP = 1    // every triplet becomes an entry; equal pairs stay adjacent in source order
};

struct CooConfig {
    int duplicates;   // COO_SUM or COO_KEEP
    int reserved;     // 0
    CooConfig() : duplicates(COO_SUM), reserved(0) {}
};

struct CooResult {
    int   error_code;     // SpMVError as int
    int   nnz_out;        // entries of C
    int   combined;       // n - nnz_out: triplets folded into an earlier one (0 with COO_KEEP)
    int   passes;         // radix passes run: the 8-bit digits of the key in which two triplets differ
    int   tile_entries;   // entries one workgroup sorts per pass (the geometry of the device sort; set on every call)
    int   launches;       // kernel launches of the call
    float elapsed_ms;     // device-event time from before the validation pass until C's arrays are complete
    CooResult() : error_code(0), nnz_out(0), combined(0), passes(0), tile_entries(0), launches(0), elapsed_ms(0.0f) {}
};

// The sorted order of one assembly, kept on the device so that csr_coo_refill can write new values into C's pattern.
// It holds the n source positions in sorted order and, for COO_SUM, the nnz_out + 1 segment starts, with num_rows,
// num_cols, n, nnz_out and the mode.  Device footprint: 4 * n bytes, plus 4 * (nnz_out + 1) bytes with COO_SUM.
struct CooPlan;

// The definition, on HOST arrays.  Input: n triplets (rows[p], cols[p], vals[p]), 0 <= p < n, in any order, repeats
// allowed, for a num_rows x num_cols matrix.
//   1. The triplets are ordered by (row, column) with a stable sort: equal (row, column) pairs keep ascending p.
//   2. COO_SUM (the default): each run of equal (row, column) becomes one entry whose value is
//      s = vals[p0]; s += vals[p1]; s += vals[p2]; ... in fp32, left to right in ascending p.  The sum starts from the
//      first value, not from 0.0f, so a pair that occurs once keeps its bits: -0.0, NaN payloads and explicit zeros
//      are kept.  A sum that comes to zero is kept as an explicit zero.  IEEE 754 leaves the sign and payload of a NaN
//      that an addition returns to the implementation (inf + -inf is 0xFFC00000 on x86 and 0x7FC00000 on gfx950), so
//      the definition fixes them: a run of TWO OR MORE values whose sum is a NaN gives the quiet NaN 0x7FC00000.
//   3. COO_KEEP: every triplet becomes an entry, equal pairs adjacent in source order; nnz_out == n.  These are the
//      duplicate-tolerant rows that csr_transpose_gpu and csr_permute_gpu accept.
//   4. row_ptrs[r] = the number of output entries with row < r.  Empty rows are allowed anywhere, first and last
//      included.
// This is what A[i, j] += v in source order gives on a host; it is sequential on purpose, so that the bits are defined
// and the device can be held to them.  C owns new host arrays (C->nnz is the entry count); a device copy it held is
// released.
// Checks, in this order, C untouched when one fails: null C, or n > 0 with a null array -> INVALID_ARGUMENT; a negative
// size -> INVALID_DIMENSION; an unknown mode or reserved != 0 -> INVALID_ARGUMENT; a row outside [0, num_rows) or a
// column outside [0, num_cols) -> INVALID_FORMAT.
int csr_from_coo_cpu(CSRMatrix* C, int num_rows, int num_cols, int n, const int* rows, const int* cols,
                     const float* vals, const CooConfig* config = nullptr);

// The same from DEVICE arrays, on the device.  C ends up as csr_transpose_gpu leaves AT: it owns new device arrays
// (what it owned before is released), its host arrays are allocated at the new size and hold no data until
// csr_from_gpu(C).  C's row_ptrs, col_indices and the bits of its values are csr_from_coo_cpu's on every run and every
// stream.  The three input arrays are only read; they may be views at any 4-byte offset into larger buffers.
//
// Device algorithm: (1) one pass validates the indices and ORs key ^ key[0] over all triplets, key = (row <<
// bits(num_cols - 1)) | col, up to 62 bits; a key of at most 32 bits is sorted as a 32-bit integer, which halves the
// bytes the sort moves (matrices up to about 64 K x 64 K).  (2) A stable LSD radix sort of (key, source position) with
// 8-bit digits; digits in which no two keys differ are skipped (result.passes).  Only the key and the 4-byte position
// move; the values are never carried.  Each workgroup counts the digits of a tile of result.tile_entries entries by
// wavefront matching, ranks the tile into LDS in digit order and writes every digit's run to global memory
// contiguously.  (3) Head flags key[t] != key[t - 1], their exclusive scan, ONE read of nnz_out, then C is allocated
// and col_indices, the segment starts and row_ptrs (a lower bound per row) are written; COO_KEEP skips the flags.
// (4) One thread per output entry walks its segment in ascending sorted slot, which is ascending source position, and
// adds left to right.  A segment is never split across lanes, which would change the bits; an entry with a very long
// run of duplicates is therefore summed by one lane at one value per step.  Finite-element duplicate counts are single
// digits; a caller with runs of thousands pays for them here, and that cost is accepted.
// No floating-point atomics, no integer atomics, no workgroup waits for another.
//
// If `plan` is non-null, *plan receives a plan for csr_coo_refill on success (it is not written otherwise); the caller
// releases it with coo_plan_destroy.
//
// Checks, in this order, with C (and *plan) untouched when one fails: null C, or n > 0 with a null array ->
// INVALID_ARGUMENT; a negative size -> INVALID_DIMENSION; an unknown mode or reserved != 0 -> INVALID_ARGUMENT; then
// ONE device pass before anything else is allocated: every row in [0, num_rows) and every column in [0, num_cols),
// else INVALID_FORMAT; allocation failure -> CUDA_MALLOC, nothing leaked.  n == 0 succeeds with an all-zero row_ptrs,
// also with num_rows == 0.  Runs on the library stream (spmv_set_stream) and returns after the build completed.
CooResult csr_from_coo_gpu(CSRMatrix* C, int num_rows, int num_cols, int n, const int* d_rows, const int* d_cols,
                           const float* d_vals, const CooConfig* config = nullptr, CooPlan** plan = nullptr);

// Recomputes ONLY C->d_values from a new value array in the same triplet order: step (4) above, one launch, no sort,
// no allocation.  The bits equal those of a fresh csr_from_coo_gpu with these values.  Calls
// csr_invalidate_gpu_cache(C), so a cached tiled plan or transpose never serves the old values (the level schedules
// cached with C are dropped with them and rebuilt on their next use).
// Checks: null plan or C, or a null d_vals with plan n > 0 -> INVALID_ARGUMENT; C's num_rows, num_cols or nnz differ
// from the plan's -> INVALID_DIMENSION; C without device arrays -> INVALID_FORMAT.  The plan does NOT re-check C's
// pattern: handing it a matrix of the same size with another pattern gives values that belong to the plan's pattern.
// Runs on the library stream and returns after it completed.
int csr_coo_refill(const CooPlan* plan, CSRMatrix* C, const float* d_vals);

// The same enqueued on `stream` without a synchronisation.
int csr_coo_refill_async(const CooPlan* plan, CSRMatrix* C, const float* d_vals, hipStream_t stream);

// Releases a plan and its device arrays; null is allowed.
void coo_plan_destroy(CooPlan* plan);

// What a plan holds, for callers that size things by it; any pointer may be null.  Null plan -> INVALID_ARGUMENT.
int coo_plan_info(const CooPlan* plan, int* num_rows, int* num_cols, int* n, int* nnz_out, int* duplicates);

// The inverse direction, CSR to COO: d_rows[p] = the row that stores entry p, for the nnz entries of the device matrix
// A (d_rows: nnz ints on the device).  With A's own d_col_indices and d_values these are triplets again, so a CSR
// matrix can be re-assembled, merged with another (concatenate the triplets), or have its duplicates combined.
// Checks: null A, or a null d_rows with nnz > 0 -> INVALID_ARGUMENT; negative sizes or missing device arrays ->
// INVALID_FORMAT; then on the device, before d_rows is written, A's structure by csr_transpose_gpu's rule
// (row_ptrs[0] == 0, non-decreasing, row_ptrs[num_rows] == nnz, every column in [0, num_cols)) -> INVALID_FORMAT.
// Runs on the library stream and returns after it completed.
int csr_row_indices_gpu(const CSRMatrix* A, int* d_rows);

} // namespace spmv

#endif
