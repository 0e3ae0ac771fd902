// tiled.h — the LDS-tiled SpMV engine ("x staged into LDS tiles"): a two-phase,
// propagation-blocking execution of y = A x for matrices whose x does not fit on chip.
// See tiled.hip for the algorithm and the two hot kernels, tiled_cells.hip and tiled_build.hip for the
// plan builder, tiled_plan.cpp for the shape rules; this is the host-side plan object.
#ifndef SPMV_AMD_TILED_H
#define SPMV_AMD_TILED_H

#include "internal.h"

#include <cstdint>
#include <mutex>
#include <vector>

namespace spmv {
namespace detail {

struct PrState;
struct CommitRider;
struct PushTargets;
struct RowMap;
struct DanglingBits;
struct PassDesc;      // tiled_layout.h

// Per-matrix bucketed copy of the entries (built once on the device, cached in the
// side table, dropped by csr_free_gpu).  The plan owns its device arrays: deleting it frees them.
struct TiledPlan {
    int num_rows = 0, num_cols = 0;
    long long nnz = 0;              // SLOTS held in cells: the short rows' entries + row-skip markers + padding
    long long entries = 0;          // of which real matrix entries
    int strip_cols = 0;             // W: x columns per LDS strip
    int tile_rows = 0;              // R: y rows per LDS tile
    int num_strips = 0, num_tiles = 0;

    // slots sorted by cell (strip-major, tile inside a strip); inside a cell by (row, column).
    // Every cell's length is a multiple of 4 slots.
    DevBuf<float>    a_val;      // [nnz]; null when the values are folded into col_weight
    DevBuf<float>    col_weight; // [num_cols] the one value every entry of a column carries, or null
    DevBuf<uint16_t> a_lcol;     // [nnz] column - strip * W.  BUILD ONLY where strip_cols <= 16384: the finished plan then
                                 // holds the columns as a_cols14 and frees this (SPMV_DEBUG=cols=u16 keeps it instead)
    DevBuf<uint8_t>  a_cols14;   // the same columns, 14 bits a slot in 448-byte blocks of 256 slots (tiled_layout.h), or null
    DevBuf<uint8_t>  a_drow;     // [nnz] row - (row of the cell's previous slot), 0..254; 255 = advance 255 rows, no entry.
                                 // BUILD ONLY: the finished plan holds the same bytes in pass order (pass_word) and frees this
    DevBuf<float>    prod;       // [nnz] phase-1 output / phase-2 input, same order
    DevBuf<int>      cells_t;    // [2 * num_tiles * num_strips]: (begin, length) pairs, tile-major
    // phase 2's work, laid out at build time (tiled_cells.hip, pass_layout_kernel): the slots of wavefront w of tile t's workgroup
    // are the passes [pass_first[16 t + w], pass_first[16 t + w + 1]), one 32-byte descriptor each
    DevBuf<int>      pass_first; // [16 * num_tiles + 1]
    DevBuf<PassDesc> pass_desc;  // [num_passes]
    DevBuf<uint32_t> pass_word;  // [64 * num_passes] the four row-delta bytes lane l of pass p adds: word 64 p + l (all kSkip past the pass's end)
    long long num_passes = 0;

    // phase-1 work items: (strip, begin, end), at most kItemEntries slots each
    DevBuf<int> items;           // [3 * num_items]
    int  num_items = 0;
    std::vector<int> strip_first_item; // HOST [num_strips + 1]: the items are sorted by strip
    // rows longer than long_row: summed by one wavefront per 512-entry chunk from the CSR arrays
    DevBuf<int>   long_rows;     // [num_long] ascending
    int    num_long = 0;
    int    long_row = 1024;         // rows with more entries than this are "long"
    DevBuf<int>   long_chunks;   // [3 * num_long_chunks] (row, begin, end) over the CSR arrays
    int    num_long_chunks = 0;
    DevBuf<int>   long_first;    // [num_long + 1] first chunk of every long row
    DevBuf<float> long_sums;     // [num_long_chunks] per-chunk partial sums of the current SpMV
    DevBuf<int>   tile_long;     // [num_tiles + 1] first long row of every tile (index into long_rows)
    const int*   csr_row_ptrs = nullptr;   // borrowed from the matrix
    const int*   csr_cols = nullptr;
    const float* csr_vals = nullptr;
    long long    csr_nnz = 0;

    // Scratch per stream.  `prod` / `long_sums` above are written by every call, so they belong to ONE stream: the
    // first that runs the plan.  A call on another stream gets its own pair (allocated on first use, kept with
    // the plan), so asynchronous calls on one matrix from different streams do not share a product stream — the
    // reference's kernels are stateless and its callers may rely on that.
    struct StreamScratch {
        hipStream_t stream;
        DevBuf<float> prod;
        DevBuf<float> long_sums;
    };
    mutable std::mutex scratch_lock;
    mutable std::mutex launch_lock;     // held across the two launches of one SpMV
    mutable bool primary_taken = false;
    mutable hipStream_t primary_stream = nullptr;
    mutable std::vector<StreamScratch> extra_scratch;

    // what the build cost (reported by bench.py)
    double    build_ms = 0.0;       // host wall clock of the build, allocations and syncs included
    long long plan_bytes = 0;       // device memory the plan holds, its local columns counted as u16 (an upper bound where packed)
    long long col_bytes = 0;        // of which local columns, as held: 2 * nnz, or the packed array's bytes (a_cols14)
};

// the (strip columns, tile rows) the engine would pick for a matrix of this shape, and whether it
// would take the matrix at all (pure host logic; exposed for tests and reports)
bool tiled_shape_for(long long rows, long long cols, long long nnz, int* strip_cols, int* tile_rows);
// the shape alone (what the builder asks; rows, cols, nnz > 0)
void choose_shape(long long num_rows, long long num_cols, long long nnz, int* strip_cols, int* tile_rows);

// true when the matrix is worth (and able) to run through the tiled engine
bool tiled_eligible(const CSRMatrix* A);
bool tiled_eligible(const ELLMatrix* A);

// builds the plan for A's device arrays (synchronises the stream a few times)
hipError_t tiled_build(const CSRMatrix* A, TiledPlan** out, hipStream_t s);
hipError_t tiled_build(const ELLMatrix* A, TiledPlan** out, hipStream_t s);   // from the ELL slabs (no long-row path)
void tiled_free(TiledPlan* plan);      // = delete: the plan's members own what it holds

// position-weighted checksums of a_val / a_lcol / pass_word / cells_t (test aid: equal plans, equal numbers)
hipError_t tiled_checksum(const TiledPlan& plan, unsigned long long out[4], hipStream_t s);

// y = A x.  hipErrorOutOfMemory: no scratch for this (additional) stream — the caller may use another kernel.
hipError_t tiled_spmv(const TiledPlan& plan, const float* d_x, float* d_y, hipStream_t s);

// PageRank step on the same plan, in two parts.
// Phase 1 for the strips [strip_begin, strip_end) — products of the entries whose columns lie there — and,
// with_long, the long rows (which read all of r_old).  A step needs every strip and the long rows exactly
// once, in any number of calls, before its finish.  No-op when state->done.
// `commit`: the previous step's pending residual commit, folded by one workgroup at the head of this launch's grid
// (CommitRider{}: none).
hipError_t tiled_pagerank_expand(const TiledPlan& plan, int strip_begin, int strip_end, bool with_long,
                                 const float* d_r_old, const PrState* d_state, const CommitRider& commit, hipStream_t s);
// Phase 2: r_new[map.at(i)] = d * (A r_old)_i + d*s/n + (1-d)/n, block partial sums of (r_new - r_old)^2
// and of r_new over dangling nodes -> block_partials [2 * plan.num_tiles]; no-op when state->done.
// `bits` (may be empty): the flags of the shard's rows as bits, read instead of d_dangling by a contiguous slice
// without push targets.
hipError_t tiled_pagerank_finish(const TiledPlan& plan, const RowMap& map, int n_global,
                                 const float* d_r_old, float* d_r_new,
                                 const unsigned char* d_dangling, const DanglingBits& bits, float damping,
                                 const PrState* d_state, double* d_block_partials,
                                 const PushTargets& push, hipStream_t s);

} // namespace detail
} // namespace spmv

#endif
