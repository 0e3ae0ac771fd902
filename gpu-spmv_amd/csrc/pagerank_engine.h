// pagerank_engine.h — the per-shard PageRank step engine shared by the
// single-GPU pagerank() and the row-sharded multi-GPU host loop (C-ABI pr_*).
#ifndef SPMV_AMD_PAGERANK_ENGINE_H
#define SPMV_AMD_PAGERANK_ENGINE_H

#include "internal.h"

#include <algorithm>

namespace spmv {
namespace detail {

// Lives in device memory; every engine kernel reads `done` first.
struct PrState {
    float dangling_sum;     // dangling mass of the current r_old
    float final_residual;   // ||r_new - r_old||_2 of the last committed step
    int   iterations;       // committed steps
    int   converged;        // residual < tolerance was observed
    int   done;             // steps after this are no-ops
    int   reserved;
};

// Peers' rank vectors (IPC-mapped device pointers) that a step also writes its new slice
// into, so that no all-gather is needed afterwards.  Passed to the kernels by value.
constexpr int kMaxPushPeers = 15;
struct PushTargets {
    float* ptr[kMaxPushPeers];
    int count = 0;
};

// Where a shard's local row i sits in the (padded) rank vector:
//     base + (i / piece) * block + i % piece
// One contiguous slice per rank: piece = everything (the default), position = base + i.  The chunked layout
// of the overlapped exchange (pagerank_dist.py): the vector is a sequence of blocks, block c holds piece c of
// EVERY rank back to back (so that one in-place all-gather per block delivers it), base = rank * piece,
// block = world * piece.
struct RowMap {
    int base = 0;
    int piece = 0x7fffffff;
    int block = 0;
    __host__ __device__ long long at(long long row) const {
        return piece == 0x7fffffff ? base + row : base + (row / piece) * block + row % piece;
    }
};

// The dangling flags of a shard's rows as bits, for the tiled engine's phase 2 on one contiguous slice: bit i of the
// array (word i / 32, bit i % 32) is the mask byte of LOCAL row i, so a tile's rows (R is a multiple of 64) start on a word
// and a step reads 1.25 MB of flags for 10 M nodes, not 10 MB; tile_count[t] is the number of set bits among tile t's
// rows, and a tile with none reads no flags at all.  Derived from the byte mask by pr_dangling_bits; the mask is a
// property of the matrix, so this holds for the shard's life.  words == nullptr: the shard has none (bytes are read).
struct DanglingBits {
    const unsigned int* words = nullptr;    // [pr_dangling_words(local_rows)]
    const int* tile_count = nullptr;        // [plan.num_tiles]
};
inline size_t pr_dangling_words(int local_rows) { return 2 * ((static_cast<size_t>(std::max(local_rows, 0)) + 63) / 64); }

// One rank's slice of the problem: local_rows consecutive rows of the n_global x n_global matrix (CSR with
// row_ptrs rebased to 0), whose nodes sit at map.at(0 .. local_rows - 1) of the rank vectors.
struct PrShard {
    int local_rows = 0;
    RowMap map;
    int n_global = 0;
    long long nnz = 0;
    const int* d_row_ptrs = nullptr;
    const int* d_cols = nullptr;
    const float* d_vals = nullptr;
    const unsigned char* d_dangling = nullptr;   // [>= n_global] 1 = dangling node
    unsigned int* d_dangling_words = nullptr;    // see DanglingBits; both null where the shard's owner keeps none
    int* d_tile_dangling = nullptr;
    bool dangling_bits_ready = false;            // pr_dangling_bits has been enqueued since the arrays were set
    PrState* d_state = nullptr;
    double* d_block_partials = nullptr;          // [2 * pr_max_blocks()]
    int lanes = 4;                               // lanes per row, from the mean row length
    int grid = 1;                                // workgroups that write block partials
    PlanRef tiled;                               // set => steps run through the LDS-tiled engine (kept alive by the shard)
    mutable int expanded_strips = 0;             // tiled engine: strips of the coming step already expanded (pr_expand)
    mutable bool expanded_long = false;          // ... and its long rows
    // Deferred commit (pr_step_commit on the tiled engine): the block partials of the last step are written but
    // not yet folded into d_state.  The next phase-1 launch on `pending_stream` carries the fold in a workgroup
    // at the head of its grid; anything else that comes next on the shard flushes it first (pr_flush).
    mutable bool commit_pending = false;
    mutable float pending_tolerance = 0.0f;
    mutable hipStream_t pending_stream = nullptr;
};

// A pending commit riding in a phase-1 launch (passed to the kernel by value); partials == nullptr: none.
struct CommitRider {
    const double* partials = nullptr;
    int num_blocks = 0;
    float tolerance = 0.0f;
    PrState* state = nullptr;
};

int pr_max_blocks();
// chooses lanes / grid; `tiled` (may be null) switches the step to the tiled engine.
// Returns the number of block-partial pairs the shard needs (size of d_block_partials / 2).
int pr_shard_prepare(PrShard* shard, PlanRef tiled);
hipError_t pr_step(const PrShard& shard, const float* d_r_old, float* d_r_new, float damping,
                   const PushTargets& push, hipStream_t s);
// Optional head start on the coming step: the caller promises that columns [0, cols_ready) of d_r_old are
// final (the rest may still be arriving); with the tiled engine, phase 1 of every strip inside that range
// that has not run yet is enqueued now.  pr_step then runs only what is left.  Without a tiled plan: no-op.
hipError_t pr_expand(const PrShard& shard, const float* d_r_old, long long cols_ready, hipStream_t s);
hipError_t pr_reduce(const PrShard& shard, double* d_sums /*[2]*/, hipStream_t s);
hipError_t pr_commit(const PrShard& shard, const double* d_sums, float tolerance, hipStream_t s);
hipError_t pr_reduce_commit(const PrShard& shard, float tolerance, hipStream_t s);   // single rank: both in one launch
// Single rank: the step, its commit deferred into the next step's phase-1 launch where the tiled engine runs
// (otherwise pr_step + pr_reduce_commit).  d_state lags by this one commit until the next step or pr_flush.
hipError_t pr_step_commit(const PrShard& shard, const float* d_r_old, float* d_r_new, float damping,
                          float tolerance, hipStream_t s);
// Enqueues a pending commit on `s` as a launch of its own (no-op when none is pending).  Every entry above other
// than a carrying pr_step does this first; callers that read d_state themselves call it before they do.
hipError_t pr_flush(const PrShard& shard, hipStream_t s);
inline void pr_drop_pending(const PrShard& shard) { shard.commit_pending = false; }
hipError_t pr_commit_gathered(const PrShard& shard, const float* d_gathered, int world, long long stride,
                              long long shard_len, float tolerance, hipStream_t s);
// Fills the shard's d_dangling_words / d_tile_dangling from d_dangling on `s` (no-op without the arrays, without a
// tiled plan, or on a chunked map: only the contiguous-slice branch of phase 2 reads them).
hipError_t pr_dangling_bits(PrShard* shard, hipStream_t s);
hipError_t pr_fill(float* d_r, size_t n, float value, hipStream_t s);
hipError_t pr_column_sums(long long nnz, const int* d_cols, const float* d_vals, int n_cols,
                          float* d_col_sums, hipStream_t s);
hipError_t pr_mask_from_column_sums(const float* d_col_sums, int n, unsigned char* d_mask,
                                    unsigned long long* d_count, hipStream_t s);

} // namespace detail
} // namespace spmv

#endif
