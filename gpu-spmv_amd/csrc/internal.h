// internal.h — helpers shared by the library's translation units (not installed).
#ifndef SPMV_AMD_INTERNAL_H
#define SPMV_AMD_INTERNAL_H

#include "spmv/common.h"
#include "spmv/csr_matrix.h"
#include "spmv/ell_matrix.h"
#include "spmv/spmv.h"

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

namespace spmv {
namespace detail {

inline int code(SpMVError e) { return static_cast<int>(e); }

// ---- per-matrix auxiliary data (side table keyed by the device row_ptrs) ----
// The public structs cannot grow (callers poke the fields), so anything the
// kernels precompute for a matrix lives here and is dropped by csr_free_gpu.
struct TiledPlan;
// A plan is shared between the side table and whoever is using it (a dispatch in flight, a PageRank shard
// engine): replacing or dropping the table's entry never pulls it from under a user.
using PlanRef = std::shared_ptr<const TiledPlan>;

// Buffers of pagerank() kept with the matrix between calls (seven device allocations, a pinned mirror and
// two events per call cost more than the iterations on a large graph), plus the dangling mask, which
// depends on the matrix only.
struct PrWorkspace {
    size_t len = 0;                       // vector length everything below is sized for
    float* r[2] = {nullptr, nullptr};     // the two rank vectors
    unsigned char* mask = nullptr;        // dangling mask
    bool mask_valid = false;
    // the matrix the mask was computed for: two matrices may share one row-pointer array (every k-per-row
    // graph has the same one), and a handle's column / value arrays may be swapped under it
    const void* mask_cols = nullptr;
    const void* mask_vals = nullptr;
    long long mask_nnz = 0;
    int mask_rows = 0, mask_num_cols = 0;
    unsigned long long num_dangling = 0;
    double* partials = nullptr;           // block partial sums / normalisation scratch
    size_t partial_count = 0;
    double* sums = nullptr;               // [2]
    void* state = nullptr;                // PrState on the device
    unsigned long long* dangling_count = nullptr;
    void* pinned_state = nullptr;         // PrState[2], pinned host
    float* pinned_ranks = nullptr;        // [len] pinned host staging for the copy out: allocated by the first call that needs it
    hipEvent_t seen[2] = {nullptr, nullptr};
    bool busy = false;                    // a call is using it (a concurrent call on the same matrix allocates its own)
    void release();
};

// Device arrays of a CSR matrix a builder made (transpose_build, spgemm_build, csr_permute_gpu, ...);
// hipMalloc-owned until csr_adopt_device hands them to a CSRMatrix.
struct DeviceCsrArrays {
    int*   row_ptrs = nullptr;      // [rows + 1]
    int*   col_indices = nullptr;   // [nnz], null when nnz == 0
    float* values = nullptr;        // [nnz], null when nnz == 0
    // row_ptrs [row_ptr_count] always, the other two [nnz] only for nnz > 0.  On a failure everything held is released
    // and the HIP error cleared; the caller maps it to its own SpMVError.
    hipError_t alloc(long long row_ptr_count, long long nnz);
    // the other two alone, for a builder whose row pointers come out of a scan before nnz is known
    hipError_t alloc_entries(long long nnz);
    void release();
};
// releases the arrays at the end of the scope, unless they were handed over (csr_adopt_device empties them)
struct ReleaseOnExit {
    DeviceCsrArrays* arrays;
    ~ReleaseOnExit() { arrays->release(); }
};

// sptrsv_csr's level schedule of one triangle (sptrsv_host.cpp): structure only, never the values.  Shared between
// the side table and the solves in flight, like a tiled plan.
struct SptrsvSchedule {
    struct Group {                   // one launch
        int level_begin, level_end;  // levels [level_begin, level_end)
        int rows;                    // rows of the widest level in it
    };
    int* d_level_ptr = nullptr;      // [num_levels + 1]
    int* d_order = nullptr;          // [num_rows] rows by level, ascending row index within a level
    int  num_levels = 0;
    std::vector<Group> groups;       // level_end - level_begin > 1 only for narrow levels: one workgroup walks them
    long long triangle_nnz = 0;      // stored entries inside the triangle, diagonal included
    int  first_missing_diagonal = -1;
    int  first_unsorted_row = -1;    // lowest row whose columns are not strictly ascending, or -1 (ilu0_csr needs none)
    // LOWER schedules of a sorted matrix with every diagonal: a row holding a stored (i,k) whose (k,i) is not stored,
    // or -1 when the pattern is structurally symmetric (ic0_csr needs that); -1 where it was not tested
    int  one_sided_row = -1;
    // built by sptrsv_analysis.hip: the same ints, except that one_sided_row is the LOWEST row that stores an (i,k),
    // k != i, whose (k,i) is not stored (the host pass may name another row of the same pattern; the sign agrees)
    bool built_on_device = false;
    // what it was built from (the transpose cache's rule)
    const void* row_ptrs = nullptr;
    const void* cols = nullptr;
    long long nnz = 0;
    int num_rows = 0, num_cols = 0, uplo = 0;
    ~SptrsvSchedule();
};
using ScheduleRef = std::shared_ptr<const SptrsvSchedule>;

struct CsrAux {
    PrWorkspace pagerank;
    // sptrsv_csr: one schedule per triangle, built on first use
    std::mutex sptrsv_lock;          // one analysis per matrix when threads race on the first call
    std::shared_ptr<const SptrsvSchedule> sptrsv[2];
    // row-length statistics computed once (host scan or device reduction)
    bool   have_stats = false;
    CSRStats stats{};
    // merge-path partition: first row of every tile, built on first use
    int*   d_tile_rows = nullptr;    // [num_tiles + 1]
    int    num_tiles = 0;
    int    tile_items = 0;
    // merge-path carry-out slots: written by every call, so they belong to the first stream that uses them;
    // a call on another stream gets its own pair (extra_carry), like the tiled plan's product stream
    int*   d_carry_row = nullptr;    // [num_tiles]
    float* d_carry_val = nullptr;    // [num_tiles]
    struct MergeCarry {
        hipStream_t stream;
        int* row;
        float* val;
    };
    std::mutex merge_lock;           // guards the fields below and the tile + fix-up pair of launches
    bool carry_taken = false;
    hipStream_t carry_stream = nullptr;
    std::vector<MergeCarry> extra_carry;
    // spmv_csr_multi's merge path (spmm.hip): its own partition and k-wide carry slots, never shared with the
    // single-vector fields above.  A stream keeps its pair (up to eight streams per matrix; beyond that a call
    // borrows one from the stream-ordered allocator); a pair grows, after a synchronisation of its stream, when a
    // call asks for more columns than it holds.
    int*   d_multi_tile_rows = nullptr;   // [multi_num_tiles + 1]
    int    multi_num_tiles = 0;
    struct MultiCarry {
        hipStream_t stream;
        int* row;      // [multi_num_tiles]
        float* val;    // [multi_num_tiles * cap_k]
        int cap_k;
    };
    std::vector<MultiCarry> multi_carry;
    std::mutex multi_lock;           // guards the multi fields and the tile + fix-up pair of launches
    // spmv_csr_transpose: the matrix's device transpose, built on first use, and what it was built from (two
    // matrices may share one row-pointer array, and a handle's column / value arrays may be swapped under it).
    // The transpose is a matrix of its own: its merge partition, tiled plan and promotion count live in ITS aux
    // entry, dropped with it (the deleter is csr_free_gpu).
    std::mutex transpose_lock;       // one build per matrix when threads race on the first call
    std::shared_ptr<CSRMatrix> transpose;
    const void* transpose_cols = nullptr;
    const void* transpose_vals = nullptr;
    long long transpose_nnz = 0;
    int transpose_rows = 0, transpose_num_cols = 0;
    // LDS-tiled engine: bucketed copy of the entries, built on first use (tiled.h)
    std::shared_ptr<TiledPlan> tiled;
    bool tiled_failed = false;       // build failed once (e.g. out of memory): do not retry
    // spmv_csr() calls on this matrix that named a REORDERING kernel (VECTOR_CSR / MERGE_PATH) without use_texture:
    // from the call after tiled_promotion() of them on, the plan is built and they take the tiled engine too
    std::atomic<int> reorder_calls{0};
    // plans thrown away because another matrix over the same row-pointer array (the side table's key) wanted one: past
    // two, promotion stops building for this key — callers that alternate such matrices would rebuild on every call
    int plan_replacements = 0;
    // fsai_csr (fsai_host.cpp), kept with the G it built for fsai_csr_numeric: the longest row of the pattern (0: not
    // known) and the device word the bad_row scan folds into, so that a refill allocates and reads back nothing else
    int fsai_max_row = 0;
    unsigned* d_fsai_word = nullptr;
};

// Ski-rental promotion: the reference's own callers spell the kernel and never set use_texture
// (benchmarks/main.cu:52-56 {VECTOR_CSR, 256, false}; src/pagerank.cu:89-90), which on a large matrix costs 5x the tiled
// engine's time per call.  After this many direct calls on one eligible matrix — about one plan build's worth of time,
// the rule pagerank() applies to itself — the next call builds the plan (outside its timed region) and every later
// VECTOR_CSR / MERGE_PATH call on the matrix takes the tiled route.  0 = never (SPMV_TILED_PROMOTE=0 sets that at start).
// SCALAR_CSR and spmv_ell without use_texture keep their CPU-order contract and never promote.
int tiled_promotion();
void set_tiled_promotion(int calls);

// the matrix's tiled plan (built on first call), or nullptr when not eligible / not buildable
PlanRef tiled_plan_for(const CSRMatrix* A, hipStream_t s);
// the plan only if the matrix already holds a valid one (never builds)
PlanRef tiled_plan_if_cached(const CSRMatrix* A);

CsrAux* aux_lookup(const void* key, bool create);
void    aux_drop(const void* key);

struct EllAux {
    bool have_nnz = false;
    long long actual_nnz = 0;   // non-padding slots, counted once on the device
    std::shared_ptr<TiledPlan> tiled; // LDS-tiled engine plan built from the slabs (use_texture)
    bool tiled_failed = false;
};
PlanRef tiled_plan_for(const ELLMatrix* A, hipStream_t s);
EllAux* ell_aux_lookup(const void* key, bool create);
void    ell_aux_drop(const void* key);

// ---- debugging / tuning overrides: ONE environment variable ----
// SPMV_DEBUG="key=value,key,..." (read at every use: tests change it between plan builds).  Keys:
//   min_cols=N, min_nnz=N      size thresholds of the LDS-tiled engine (tests push small matrices through it)
//   strip=W, tile=R, item=N    plan shape overrides: strip columns (4096..32768), tile rows (multiple of 64), slots per phase-1 item
//   long_factor=N, long_cap=N  long-row limit = min(long_cap, long_factor * strips)
//   cols=u16                   the plan keeps its local columns as u16 per slot on every strip width (default: packed to
//                              14 bits wherever strip columns <= 16384, tiled_layout.h)
//   rank=plain                 ranking pass of the plan build by comparison (no stable binning)
//   place=scattered            placing pass of the plan build entry by entry (no LDS staging)
//   pr_plan_after=N            direct steps pagerank() takes before it builds a plan (default 4)
//   pr_copy=pageable           pagerank() copies its result into a pageable array (no pinned pool)
//   sptrsv_lanes=N             lanes per row of sptrsv_csr with ordered = 0 (1, 2, 4, ... 64; anything else is ignored)
//   sptrsv_analysis=device     every implicit level analysis (the first solve or factorisation per matrix and triangle,
//                              sptrsv_analyze) is built on the device, as sptrsv_analyze_device does; anything else:
//                              on the host
//   analysis_lanes=N           lanes per row of the device-side level analysis's kernels (1, 2, 4, ... 64; anything else
//                              is ignored)
//   ilu0_lanes=N               lanes per row of ilu0_csr (1, 2, 4, ... 64; anything else is ignored)
//   ic0_lanes=N                lanes per row of ic0_csr (1, 2, 4, ... 64; anything else is ignored)
//   fsai_lanes=N               lanes per row of fsai_csr's numeric kernel (1, 2, 4, ... 64; anything else is ignored)
//   fsai_class=C               LDS capacity class of that kernel (4, 8, 16, 32, 64; anything else is ignored); a class
//                              below the longest pattern row is INVALID_ARGUMENT
//   spgemm_lanes=N             lanes per row of C in spgemm_csr (1, 2, 4, ... 64; anything else is ignored)
//   spgemm_class=N             accumulator class every row of spgemm_csr takes (1 .. 5); a row too large for it takes
//                              the first class that holds it
//   spgemm_dense_groups=G      workgroups (and scratch slices) of spgemm_csr's dense class, instead of the scratch cap
//   amg_lanes=N                lanes per row (and per aggregate) of every level of the AMG V-cycle (1, 2, 4, ... 64;
//                              anything else is ignored)
//   mis_lanes=N                lanes per row of the MIS-2 aggregation's kernels (1, 2, 4, ... 64; anything else is ignored)
//   ppr_lanes=N                lanes per row of pagerank_personalized's step (1, 2, 4, ... 64; anything else is ignored)
//   add_lanes=N                lanes per row of csr_add and csr_add_numeric (1, 2, 4, ... 64; anything else is ignored)
//   bsr_lanes=N                lanes per block row of bsr_from_csr_gpu, bsr_from_csr_numeric, csr_block_count_gpu and
//                              of spmv_bsr's lane-group kernel (1, 2, 4, ... 64; anything else is ignored)
//   bsr_tri_lanes=N            lanes per block row of bsr_ic0 and of sptrsv_bsr with ordered = 0, cg_solve_bsr_ic's solves
//                              included (1, 2, 4, ... 64; anything else is ignored)
// Everything else the library reads from the environment is listed in INTEGRATION.md.
bool debug_option(const char* key, long long* value = nullptr, char* text = nullptr, size_t text_size = 0);
// the same "key=value,key" syntax for another variable's value (SPMV_MULTI_GPU); `list` may be null
bool list_option(const char* list, const char* key, long long* value = nullptr, char* text = nullptr, size_t text_size = 0);
inline long long debug_number(const char* key, long long fallback) {
    long long v = 0;
    return debug_option(key, &v) ? v : fallback;
}
bool debug_is(const char* key, const char* expected);
// the value of one of the "..._lanes" keys where it names a lane count (1, 2, 4, ... 64); 0 where the key is absent
// or holds anything else, and the caller makes its own pick
inline int forced_lanes(const char* key) {
    long long forced = 0;
    if (debug_option(key, &forced) && forced >= 1 && forced <= 64 && (forced & (forced - 1)) == 0) {
        return static_cast<int>(forced);
    }
    return 0;
}

// ---- launch layer (kernels.hip) ----
// All return hipError_t from the launch; none synchronise.
hipError_t launch_csr_scalar(const CSRMatrix* A, const float* d_x, float* d_y, hipStream_t s);
hipError_t launch_csr_vector(const CSRMatrix* A, const float* d_x, float* d_y,
                             int lanes_per_row, hipStream_t s);
int vector_ldsx_grid(const CSRMatrix* A);      // 0 = x-in-LDS variant not worthwhile for this matrix
hipError_t launch_csr_vector_ldsx(const CSRMatrix* A, const float* d_x, float* d_y, int lanes_per_row,
                                  int grid, hipStream_t s);
hipError_t launch_csr_merge(const CSRMatrix* A, CsrAux* aux, const float* d_x, float* d_y,
                            hipStream_t s);
hipError_t prepare_csr_merge(const CSRMatrix* A, CsrAux* aux, hipStream_t s);   // the merge tile table, ahead of a timed call
hipError_t launch_ell(const ELLMatrix* A, const float* d_x, float* d_y, hipStream_t s);
// multi-vector kernels (spmm.hip): X num_cols x k, Y num_rows x k, row-major, leading dimensions ldx / ldy
hipError_t launch_csr_multi_zero(const CSRMatrix* A, float* d_Y, int ldy, int k, hipStream_t s);
hipError_t launch_csr_multi_rows(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                 hipStream_t s);     // CPU summation order
hipError_t launch_csr_multi_vector(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                   hipStream_t s);
hipError_t launch_csr_multi_merge(const CSRMatrix* A, CsrAux* aux, const float* d_X, int ldx, float* d_Y, int ldy,
                                  int k, hipStream_t s);
hipError_t prepare_csr_multi_merge(const CSRMatrix* A, CsrAux* aux, int k, hipStream_t s);  // ahead of a timed call
void release_multi_merge(CsrAux* aux);
hipError_t launch_fill_zero(float* d_y, size_t n, hipStream_t s);
// device transpose (transpose.hip): validates A (INVALID_FORMAT before anything is allocated), then builds A^T on
// `s` and returns after the build completed, its scratch freed.  The caller owns *out on SUCCESS.
int transpose_build(const CSRMatrix* A, DeviceCsrArrays* out, hipStream_t s);

// ---- the build layer: what the routines that build a CSR matrix share (csr_build.hip, csr_matrix.cpp; §4.27) ----
// How a device builder hands its result over (csr_matrix.cpp; csr_transpose_gpu's rule for AT): M's old device arrays and
// cached data are dropped, it owns *arrays from now on (*arrays is left empty), and its host arrays are allocated at the
// new size without data.  The shape is passed by value: M may be the builder's input (csr_transpose_gpu(A, A)).
void csr_adopt_device(CSRMatrix* M, int rows, int cols, int nnz, DeviceCsrArrays* arrays);
// How a host twin hands its result over: M's device arrays, if it has any, are dropped with their cached data (a device
// copy would be stale; csr_free_gpu is not called for a handle without device pointers, whose owns_device_memory stays
// as it is), its old host arrays are freed when it owns them, and it owns the three new[]-allocated arrays from now on.
void csr_adopt_host(CSRMatrix* M, int rows, int cols, int nnz, int* row_ptrs, int* col_indices, float* values);
// the same from vectors (nnz = col_indices.size()): copied first, so a failed allocation leaves M untouched
void csr_adopt_host(CSRMatrix* M, int rows, int cols, const std::vector<int>& row_ptrs,
                    const std::vector<int>& col_indices, const std::vector<float>& values);
// The hierarchical exclusive scan (tiles of 4096, 256 threads): device_scan_levels(n) gives the level sizes n,
// ceil(n / 4096), ... 1; device_exclusive_scan scans data[0, n) in place on `s`, with `sums` holding
// device_scan_sums(levels) ints of scratch; device_scan_launches(levels) is the number of kernels it launches
std::vector<long long> device_scan_levels(long long n);
long long device_scan_sums(const std::vector<long long>& levels);
int device_scan_launches(const std::vector<long long>& levels);
hipError_t device_exclusive_scan(int* data, const std::vector<long long>& levels, int* sums, hipStream_t s);
// The structure check (csr_transpose_gpu's rule: row_ptrs[0] == 0, non-decreasing, row_ptrs[rows] == nnz, every column
// in [0, num_cols)).  enqueue_validate: *d_flag (zeroed by the caller) becomes 1 when A is malformed; not waited for.
// structure_checked: run on `s` and waited for: 0, or the code of CUDA_MALLOC (no flag word), KERNEL_LAUNCH (a call
// failed; the HIP error is cleared) or INVALID_FORMAT
hipError_t enqueue_validate(const CSRMatrix* A, int* d_flag, hipStream_t s);
int structure_checked(const CSRMatrix* A, hipStream_t s);
// row_of[p] = the row that holds entry p of validated row pointers, for nnz > 0 (256 entries per workgroup)
hipError_t launch_expand_rows(const int* rp, int rows, long long nnz, int* row_of, hipStream_t s);
// out[i] = i for i in [0, n), `grid` workgroups of 256 threads striding
hipError_t launch_iota(long long n, int* out, int grid, hipStream_t s);

// The two rules for "the matrix is on the device".  Which error a half-uploaded matrix gets is tested behaviour: a
// site whose rule differs from both in any input keeps its own spelling, with a comment that says what differs.
// STRICT — the solvers, eigs_sym and pagerank_personalized (their callers have returned for num_rows == 0 already):
// d_row_ptrs always, the other two for nnz > 0; a negative nnz counts as no entries, a negative num_rows fails.
inline bool device_arrays_strict(const CSRMatrix* M) {
    return M->num_rows >= 0 && M->d_row_ptrs && (M->nnz <= 0 || (M->d_col_indices && M->d_values));
}
// LENIENT — csr_transpose_gpu's rule, for the builders that take a matrix without rows (the transpose, spgemm_csr,
// csr_add, csr_scale_gpu, csr_diagonal_gpu, csr_row_indices_gpu): no negative size, the arrays only where there are
// rows (and, for the other two, entries), and no entries without rows (row_ptrs[0] == 0 != nnz).
inline bool device_arrays_lenient(const CSRMatrix* M) {
    if (M->num_rows < 0 || M->num_cols < 0 || M->nnz < 0) return false;
    if (M->num_rows > 0 && (!M->d_row_ptrs || (M->nnz > 0 && (!M->d_col_indices || !M->d_values)))) return false;
    return M->num_rows > 0 || M->nnz == 0;
}

// ---- small host helpers of the builders ----
// clears the HIP error, stores the code in the result struct and returns it
template <typename Result>
int fail(Result* result, SpMVError e) {
    (void)hipGetLastError();
    result->error_code = code(e);
    return result->error_code;
}
inline int fail(SpMVError e) {
    (void)hipGetLastError();
    return code(e);
}
// four events of one call (symbolic and numeric begin / end), destroyed with it
struct Events {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    Events() {
        for (hipEvent_t& x : e) ok = hipEventCreate(&x) == hipSuccess && ok;
    }
    ~Events() {
        for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x);
    }
    Events(const Events&) = delete;
    Events& operator=(const Events&) = delete;
};
// the last launch's error and the stream's, as a status (waits for `s`)
inline int stream_finished(hipStream_t s) {
    const bool ok = hipGetLastError() == hipSuccess;
    if (hipStreamSynchronize(s) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}
// spgemm_csr's accumulator classes (spgemm.hip, spgemm_host.cpp): classes 1 .. kSpgemmClasses - 1 are LDS hash tables
// of kSpgemmSlots slots (a power of two; a row may fill half of them), the last class is the dense accumulator
constexpr int kSpgemmClasses = 5;
constexpr int kSpgemmSlots[kSpgemmClasses - 1] = {32, 256, 2048, 16384};
// sparse triangular solve (sptrsv.hip): the launches of one solve, one per group of the schedule, in stream order
// (device_common.h launch_level_groups); kSptrsvNarrowRows is the widest level a single workgroup takes inside a run
// of levels.  What the drivers over a schedule share (predicates, the timed, async and analyze shapes) is in
// level_driver.h.
constexpr int kSptrsvNarrowRows = 256;
constexpr int kSptrsvMaxRunLevels = 8192;     // levels per single-workgroup launch at most (bounds one kernel's time)
hipError_t launch_sptrsv(const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_b, float* d_x, int uplo,
                         int unit_diagonal, bool ordered, int lanes_per_row, hipStream_t s);
// The k-wide solve (sptrsv_multi.hip): the same launches for k columns at once.  Column c of row i lives at
// base + (c / w) * window + i * ld + c % w, w = 4 or 8 accumulators per lane: a caller's num_rows x k array has
// window = w, the windowed workspace of cg_multi.hip (num_rows x w arrays one after another) window = num_rows * w
// and ld = w.  B may be X (the same ld and window): the solve in place.
struct SptrsvMultiArrays {
    const float* B;
    int ldb;
    long long b_window;
    float* X;
    int ldx;
    long long x_window;
    int k;                           // columns solved: [0, k)
    int w;                           // 4 or 8
};
hipError_t launch_sptrsv_multi(const SptrsvSchedule& schedule, const CSRMatrix* A, const SptrsvMultiArrays& arrays,
                               int uplo, int unit_diagonal, bool ordered, int lanes_per_row, hipStream_t s);
// the schedule cache of sptrsv_host.cpp for the callers that solve or factor with it (factor0_host.cpp, bicgstab.hip):
// checks 2-4 of sptrsv.h (not square, no rows, missing device arrays); A's `uplo` schedule, built and cached when it
// is not there (*analysis_ms = the host time of a build, 0 for a cache hit); the lanes per row of an ordered = 0 solve
int sptrsv_check_matrix(const CSRMatrix* A, bool* nothing_to_do);
int sptrsv_schedule_for(const CSRMatrix* A, int uplo, hipStream_t stream, ScheduleRef* out, float* analysis_ms);
int sptrsv_lanes_for(const SptrsvSchedule& schedule);
// The level analysis on the device (sptrsv_analysis.hip), for A that passed sptrsv_check_matrix and
// has rows: structure_checked's rule first (INVALID_FORMAT before any kernel follows a row pointer or a column), then
// d_level_ptr, d_order, num_levels, triangle_nnz, first_missing_diagonal, first_unsorted_row, one_sided_row and
// built_on_device of *out, waited for on `s`; *level_ptr is the host copy of d_level_ptr the grouping needs.  On an
// error *out owns nothing.
int sptrsv_analysis_device(const CSRMatrix* A, int uplo, hipStream_t s, SptrsvSchedule* out,
                           std::vector<int>* level_ptr);
// The zero-fill factorisations (factor0.hip): the launches of one factorisation over A's LOWER schedule, in stream
// order, from d_a (A's values) into d_out (may be the same array); then, when d_pivot is not null, the scan of the
// finished diagonal that folds the lowest row with a bad pivot into it (an unsigned min; preset to all ones).
//   ILU0  the whole row: L left of the diagonal, U on and right of it; a bad pivot is zero or not finite
//   IC0   from the lower triangle and diagonal of d_a: L on and left of the diagonal, L^T right of it; a bad pivot is
//         not > 0 or not finite
enum class Factor0Kind { ILU0, IC0 };
hipError_t launch_factor0(Factor0Kind kind, const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_a,
                          float* d_out, int lanes_per_row, unsigned* d_pivot, hipStream_t s);
// A row of the square, valid CSR pattern (rows strictly ascending, every diagonal stored) that holds one side only of
// some pair (i,k) / (k,i), or -1 when the pattern is structurally symmetric.  One pass: row k's upper entries must be
// met in their stored order as the rows below it are walked downwards.
inline int one_sided_row(int n, const int* row_ptrs, const int* cols) {
    std::vector<int> next(static_cast<size_t>(n));      // first upper position of row k not yet matched
    for (int k = 0; k < n; ++k) {
        int p = row_ptrs[k];
        while (p < row_ptrs[k + 1] && cols[p] <= k) ++p;
        next[k] = p;
    }
    for (int i = 0; i < n; ++i) {
        for (int p = row_ptrs[i]; p < row_ptrs[i + 1] && cols[p] < i; ++p) {
            const int k = cols[p];
            if (next[k] >= row_ptrs[k + 1] || cols[next[k]] != i) return i;
            ++next[k];
        }
    }
    for (int k = 0; k < n; ++k) {
        if (next[k] != row_ptrs[k + 1]) return k;
    }
    return -1;
}
hipError_t launch_ell_from_csr(const CSRMatrix* csr, int width, int* d_ell_cols, float* d_ell_vals,
                               hipStream_t s);
hipError_t device_count_ell_nnz(const ELLMatrix* A, long long* out, hipStream_t s);
hipError_t device_row_stats(const int* d_row_ptrs, int num_rows, int* max_out, int* min_out,
                            hipStream_t s);

// lanes-per-row choice for VECTOR_CSR from the mean row length (wave64 tuning)
int pick_lanes_per_row(float avg_nnz_per_row);

// Device memory with an owner: freed when the owner goes, on every path.  Move-only; pass .get() to a kernel.
struct DevFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <typename T>
using DevBuf = std::unique_ptr<T, DevFree>;
// max(count, 1) elements of T; whatever *out held before is freed
template <typename T>
hipError_t dev_alloc(DevBuf<T>* out, long long count) {
    T* p = nullptr;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), static_cast<size_t>(std::max<long long>(count, 1)) * sizeof(T));
    out->reset(e == hipSuccess ? p : nullptr);
    return e;
}

// timing helper: a cached event pair per thread
struct EventPair {
    hipEvent_t start = nullptr;
    hipEvent_t stop = nullptr;
};
EventPair& thread_events();

hipStream_t current_stream();

// hipMalloc that is also legal while some stream of this thread is being captured into a hipGraph (the
// thread's capture mode is switched to "relaxed" around the call): per-stream scratch is allocated at a
// stream's first call on a matrix, and that first call may well be the one a graph capture records.
hipError_t malloc_any_time(void** ptr, size_t bytes);

// roctx range around a host-side phase (plan build, dispatch, PageRank step): shows up under
// `rocprofv3 --marker-trace`, costs two indirect calls when a profiler has loaded the roctx library and
// nothing measurable otherwise (the library is looked up once, lazily; no link-time dependency).
struct TraceRange {
    explicit TraceRange(const char* name);
    ~TraceRange();
    TraceRange(const TraceRange&) = delete;
    TraceRange& operator=(const TraceRange&) = delete;
private:
    bool open_;
};

} // namespace detail
} // namespace spmv

#endif
