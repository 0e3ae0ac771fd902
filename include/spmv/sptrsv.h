// spmv/sptrsv.h — sparse triangular solve T x = b with level scheduling, T a triangle of a square CSR matrix.
//
// The primitive under Gauss-Seidel, IC(0) and ILU(0) preconditioners: rows depend on each other, so the rows are
// sorted into dependency levels once per (matrix, triangle), on the host or (sptrsv_analyze_device) on the device, and a solve is a short sequence of
// launches in which every row of a level is independent (gpu-spmv_amd/csrc/sptrsv.hip).
#ifndef SPMV_SPTRSV_H
#define SPMV_SPTRSV_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct SpTRSVConfig {
    enum Uplo { LOWER = 0, UPPER = 1 };
    enum Diag { NON_UNIT = 0, UNIT = 1 };
    int uplo;      // Uplo: which triangle of A is T; entries on the other side of the diagonal are ignored
    int diag;      // Diag
    int ordered;   // 1: one lane per row, the summation order of sptrsv_cpu_csr (bit-identical); 0: 1-64 lanes per row
    int reserved;  // 0
    SpTRSVConfig() : uplo(LOWER), diag(NON_UNIT), ordered(0), reserved(0) {}
};

struct SpTRSVResult {
    int   error_code;     // SpMVError as int
    int   num_levels;     // dependency levels of the triangle
    int   launches;       // kernel launches of one solve (groups of levels)
    int   lanes_per_row;  // lanes that shared a row in this solve
    float analysis_ms;    // host time of the analysis this call ran; 0 when the cached schedule was used
    float elapsed_ms;     // device-event time of the solve launches only
    SpTRSVResult() : error_code(0), num_levels(0), launches(0), lanes_per_row(0), analysis_ms(0.0f),
                     elapsed_ms(0.0f) {}
};

// Solves T x = b on the device, T the config->uplo triangle of the square matrix A (resident on the device:
// csr_to_gpu / csr_wrap_device).  Entries of A on the other side of the diagonal are skipped, not an error: a full
// SPD or non-symmetric matrix can be solved with either of its triangles without a second copy.  d_b, d_x:
// num_rows floats (device).  config == nullptr: SpTRSVConfig().
//
// Diagonal: with NON_UNIT the diagonal of row i is the fp32 sum of its stored (i,i) entries in storage order (the
// rule of cg.h); with UNIT stored (i,i) entries are ignored and the diagonal is 1.  A stored diagonal whose value is
// zero is not an error: the row gets the IEEE quotient (inf or NaN), exactly as sptrsv_cpu_csr produces, and the rows
// that depend on it inherit it.
//
// Aliasing: d_b == d_x (the solve in place) is allowed: row i reads b_i before it writes x_i, and no other row
// touches index i.  Any other overlap of the two ranges is INVALID_ARGUMENT.
//
// Checks, in this order, before any device work; nothing is written to d_x when one fails:
//   null A / d_b / d_x -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS;
//   missing device arrays -> INVALID_FORMAT; uplo / diag / ordered out of range -> INVALID_ARGUMENT; d_b and d_x
//   overlapping without being equal -> INVALID_ARGUMENT; then from the analysis: row_ptrs not monotone (or outside
//   [0, nnz]) or a column index outside [0, num_rows) -> INVALID_FORMAT; NON_UNIT and a row without a stored
//   diagonal entry -> INVALID_ARGUMENT.
//
// Analysis: level(i) = 0 when row i has no off-diagonal entry inside the triangle, else 1 + the largest level of
// the rows those entries name (sptrsv_levels below).  The first call per (matrix, uplo) reads row_ptrs and
// col_indices back from the device once, computes the levels on the host, uploads the schedule and keeps it with the
// matrix; it synchronises the stream, so make it (or sptrsv_analyze) outside a graph capture and outside a timed
// region.  sptrsv_analyze_device (below) builds the same schedule without the read-back, and SPMV_DEBUG=
// sptrsv_analysis=device makes every first call do so.  The schedule is found again by the matrix's row-pointer and column arrays, its dimensions, nnz and uplo;
// LOWER and UPPER schedules live side by side.  csr_invalidate_gpu_cache / csr_free_gpu drop them.  The schedule
// holds STRUCTURE only: the values, the diagonal included, are read from A's arrays by every solve, so rewriting
// d_values in place (a refactorisation with the same pattern) needs no invalidation.  Rewriting d_row_ptrs or
// d_col_indices in place does.
//
// Launches: consecutive levels of at most 256 rows each are one launch of a single workgroup that walks them with a
// workgroup barrier in between; a wider level is a launch of its own over its rows.  The order between launches is
// stream order: no workgroup ever waits for another one, so no input can make a solve hang.
//
// Numerics: fp32.  ordered = 1: one lane per row; s = 0.0f, then s = s + a_ij * x_j (product rounded, then sum
// rounded) over the triangle's off-diagonal entries in storage order, x_i = (b_i - s) / d_i: bit-identical to
// sptrsv_cpu_csr.  ordered = 0 (default): 1, 2, 4, ... or 64 lanes per row, from the mean number of stored entries
// per row inside the triangle; each lane accumulates its strided share with fused multiply-adds and the partial sums
// are folded by a fixed butterfly: no atomics, the same bits on every run and every stream.  The diagonal keeps the
// storage-order rule at every lane count.
SpTRSVResult sptrsv_csr(const CSRMatrix* A, const float* d_b, float* d_x, const SpTRSVConfig* config = nullptr);

// The same solve enqueued on `stream` without timing or a final synchronisation; returns the error code.  A first
// call per (matrix, uplo) still runs the analysis and synchronises `stream` for it: call sptrsv_analyze first.
int sptrsv_csr_async(const CSRMatrix* A, const float* d_b, float* d_x, const SpTRSVConfig* config,
                     hipStream_t stream);

// sptrsv_csr for k right-hand sides in ONE launch sequence: T X = B with d_B and d_X num_rows x k,
// row-major, on the device, leading dimensions ldb, ldx >= k (spmv_csr_multi's layout), 1 <= k <= 32.  The contract is
// bitwise: column j of X is what sptrsv_csr(A, B[:, j], ., config) writes at the same lanes_per_row, whatever the
// other columns hold (with ordered = 1 therefore sptrsv_cpu_csr's bits).  The diagonal of a row is computed once and
// shared by the columns; a zero diagonal gives each column its own IEEE quotient, and an inf or NaN of one column
// never reaches another.  The schedule is sptrsv_csr's (same cache, same key, same invalidation: a multi call after
// a single call reports analysis_ms == 0 and the other way round), the lanes are sptrsv_csr's, and num_levels,
// launches and lanes_per_row of the result equal the single-column call's: the launch count does not depend on k.
// Columns k..ldx-1 of d_X are never written; d_B is never written unless it is d_X.
//
// Aliasing: d_B == d_X with ldb == ldx is the solve in place.  Any other overlap of the ranges
// d_B[0, (num_rows - 1) * ldb + k) and d_X[0, (num_rows - 1) * ldx + k) is INVALID_ARGUMENT.
//
// Checks, in this order, before any device work; nothing is written to d_X when one fails: null A / d_B / d_X ->
// INVALID_ARGUMENT; k < 1 or k > 32 -> INVALID_ARGUMENT; ldb < k or ldx < k -> INVALID_ARGUMENT; then sptrsv_csr's
// from the dimension check on, with the overlap rule above.
SpTRSVResult sptrsv_csr_multi(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                              const SpTRSVConfig* config = nullptr);

// The same enqueued on `stream` without timing or a final synchronisation (sptrsv_csr_async's rules).
int sptrsv_csr_multi_async(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                           const SpTRSVConfig* config, hipStream_t stream);

// sptrsv_cpu_csr column by column on host arrays B and X (num_rows x k row-major, ldb, ldx >= k): column j of X is
// bit for bit sptrsv_cpu_csr on column j of B.  B == X with ldb == ldx is allowed; any other overlap of the two
// ranges -> INVALID_ARGUMENT.  Checks: null arguments, then k, then ldb / ldx (INVALID_ARGUMENT each), then
// sptrsv_cpu_csr's; X is untouched on any error.
int sptrsv_cpu_csr_multi(const CSRMatrix* A, const float* B, int ldb, float* X, int ldx, int k,
                         const SpTRSVConfig* config = nullptr);

// Builds and caches the schedule of A's `uplo` triangle ahead of a timed call (on spmv_get_stream()).  Checks as
// sptrsv_csr's for A and uplo; a missing diagonal is not an error here (a UNIT solve may follow).  num_levels,
// launches and analysis_ms of the result are filled; analysis_ms is 0 when the schedule was already there.
SpTRSVResult sptrsv_analyze(const CSRMatrix* A, int uplo);

// sptrsv_analyze with the analysis run on the device (gpu-spmv_amd/csrc/sptrsv_analysis.hip): no
// array of A crosses the bus, only the level pointers (num_levels + 1 ints) and a few counters come back.  The same
// checks in the same order and the same result fields; analysis_ms is the wall time of the build, and 0 when a
// schedule, however built, is already cached.  The schedule goes into the same cache under the same key and
// invalidation as the host-built one and every consumer (the solves, ilu0_csr, ic0_csr, the *_lu / *_ic solvers) finds
// it unchanged: level pointers, order, launches and statistics are the host analysis's ints.  Two differences: the
// structure is checked by csr_transpose_gpu's rule (row_ptrs[0] == 0 and row_ptrs[num_rows] == nnz are required, where
// the host analysis accepts any row_ptrs inside [0, nnz]), and one_sided_row (SpTRSVScheduleInfo) may name another row.
// Integer atomics only, none whose outcome depends on arrival order: the same arrays on every run and every stream.
// No workgroup waits for another; the host loop enqueues at most num_rows + 1 rounds, whatever the input.
SpTRSVResult sptrsv_analyze_device(const CSRMatrix* A, int uplo);

// What the cached schedule of (A, uplo) holds besides its arrays.  32 bytes.
struct SpTRSVScheduleInfo {
    int num_levels;
    int launches;                // kernel launches of one solve (groups of levels)
    int first_missing_diagonal;  // lowest row without a stored (i,i) entry, or -1
    int first_unsorted_row;      // lowest row whose columns are not strictly ascending, or -1
    // LOWER schedules of a matrix with sorted rows and every diagonal: a row that stores an (i,k), k != i, whose (k,i)
    // is not stored, or -1 when the pattern is structurally symmetric; -1 where it was not tested.  The device
    // analysis names the lowest such row, the host analysis the first its one pass meets: only the sign is shared.
    int one_sided_row;
    int built_on_device;         // 1: sptrsv_analyze_device (or SPMV_DEBUG=sptrsv_analysis=device) built it
    long long triangle_nnz;      // stored entries inside the triangle, diagonal included
};

// Copies the cached schedule of (A, uplo), of either origin, to host arrays: level_ptr (num_levels + 1 ints: give it
// room for num_rows + 1) and order (num_rows ints: the rows by level, ascending inside a level); either may be null.
// *info (may be null) is filled.  Builds nothing.  Checks, in this order: null A -> INVALID_ARGUMENT; uplo out of
// range -> INVALID_ARGUMENT; no schedule cached for (A, uplo) -> INVALID_ARGUMENT, and nothing is written.
int sptrsv_schedule_get(const CSRMatrix* A, int uplo, int* level_ptr, int* order, SpTRSVScheduleInfo* info);

// Host forward (LOWER) / backward (UPPER) substitution on A's HOST arrays, the counterpart of spmv_cpu_csr and the
// definition of the ordered solve: rows in ascending (LOWER) or descending (UPPER) order, per row s = 0.0f,
// s = s + a_ij * x_j in storage order over the triangle's off-diagonal entries, x_i = (b_i - s) / d_i.  b == x is
// allowed.  config->ordered is ignored.  Returns the error code: null arguments or missing host arrays ->
// INVALID_ARGUMENT, not square -> INVALID_DIMENSION, malformed arrays -> INVALID_FORMAT, NON_UNIT and a row without
// a stored diagonal -> INVALID_ARGUMENT; x is untouched on any error.
int sptrsv_cpu_csr(const CSRMatrix* A, const float* b, float* x, const SpTRSVConfig* config = nullptr);

// The analysis as a pure host function, O(nnz).  level_ptr has room for num_rows + 1 ints, order for num_rows.
// On SUCCESS: *num_levels levels; order[level_ptr[l] .. level_ptr[l + 1]) are the rows of level l in ascending row
// index (so the schedule is unique); *first_missing_diagonal (may be null) is the lowest row without a stored (i,i)
// entry, or -1.  Null pointers, num_rows < 0 or an unknown uplo -> INVALID_ARGUMENT; row_ptrs[0] < 0, decreasing
// row_ptrs or a column index outside [0, num_rows) -> INVALID_FORMAT.
int sptrsv_levels(int num_rows, const int* row_ptrs, const int* col_indices, int uplo, int* level_ptr, int* order,
                  int* num_levels, int* first_missing_diagonal);

} // namespace spmv

#endif
