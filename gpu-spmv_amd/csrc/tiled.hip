// tiled.hip — the LDS-tiled SpMV engine for matrices whose x does not fit on chip
// (the MI355X replacement of the reference's texture-cache read of x,
// src/spmv_kernels.cu:7-39; selected by SpMVConfig::use_texture).
//
// Why: on gfx950 a 4-byte gather through the vector-memory path costs one 64-byte
// fabric request and runs at <= 0.3 lane/clk/CU even from L1 (tools/gather_bench.hip:
// 295 / 185 / 61 G gathers/s from L1 / L2 / Infinity Cache), while an LDS gather runs
// at ~7 lanes/clk/CU (tools/lds_bench.hip).  So x must be gathered from LDS — but with
// e.g. 10 M columns and 16 entries per row no (row block x column strip) tile is dense
// enough to amortise loading its strip.  The engine therefore runs y = A x in two
// streaming phases over a bucketed copy of the entries (propagation blocking):
//
//   layout : slots sorted by cell = (column strip, row tile), strip-major, and by (row, column)
//        inside a cell.  Per slot: value f32, local column u16, ROW DELTA u8 (row minus the row of the
//        cell's previous slot; 255 = "advance 255 rows, no entry" for the rare larger gaps) — 7 B
//        against CSR's 8 — plus a 4-byte product slot.  Cells are padded to a multiple of 4 slots.  The row deltas are
//        kept in the order phase 2 reads them, 64 four-byte words per pass (pass_word, tiled_layout.h), not slot by slot.
//        Where a strip has at most 16384 columns the finished plan holds the local columns packed to 14 bits, 256 slots
//        in 448 bytes (a_cols14, tiled_layout.h): 1.75 B per slot instead of 2.
//   phase 1 "expand" : a workgroup loads one x strip (W = 4 K .. 32 K columns, chosen per
//        matrix = 16 .. 128 KiB) into LDS, streams its share of the strip's slots (value, local column) with
//        16-byte loads, gathers x from LDS and stores the products — same order, so
//        loads and stores are all contiguous.
//   phase 2 "reduce" : a workgroup (1024 threads) owns one row tile: R rows of DOUBLES in dynamic LDS, R a
//        multiple of 64 up to 9984 = 78 KiB, two tiles per CU, R stretched so that the tiles fill whole rounds
//        of the 512 resident workgroups.  The tile's slots are one contiguous run per strip (cell table); a
//        wavefront walks the runs of its share of the strips as one stream of 256-slot PASSES whose geometry was
//        laid out when the plan was built (pass descriptors, below): it loads 4 products (16 B) + 4 row deltas
//        (4 B) per lane, rebuilds the rows with an in-lane prefix and one DPP wavefront scan, adds each product
//        into the tile with the hardware ds_add_f64 and finally the tile is rounded to fp32 and written out with
//        coalesced stores (optionally through the fused PageRank update).  Why doubles: gfx950's ds_add_f32 runs at 0.38 lanes/clk/CU, a
//        compare-and-swap add at 3.4 but with retry storms when the tile's wavefronts meet on hot rows (round
//        1: phase 2 VALU-bound at ~225 us whatever was changed), ds_add_f64 at 3.5 (8.6 on consecutive rows)
//        with no retries (tools/lds_bench.hip, profiles/r02_lds_bench.txt, r02_phase2_counters.txt).
//   folding : when every stored entry of a column has the same bits, the value stream is dropped
//        and phase 1 gathers w_j * x_j from LDS (strip_weight_kernel, FOLD instantiation).
//   both phases walk their work lists in per-XCD contiguous slices (xcd_contiguous).
//   long rows (more than min(4096, 8 entries per strip)) would make many lanes meet on one LDS word; they are
//        left out of the cells and summed in 512-entry chunks by extra wavefronts of the phase-1 grid (direct
//        gather) into one slot per chunk; phase 2's tile start folds a long row's chunk sums in chunk order.
//   build : batches of <= ~5 K entries (consecutive rows of ONE tile).  Ranking pass: the batch is binned by
//        strip in LDS and every entry ranked inside its bin by (row, column, source index); it leaves a 4-byte
//        record per entry (position inside its group, row delta, skip markers) and the group sizes.  One thread
//        per cell then places the groups of its batches, a scan over (strip, tile) gives the cell offsets, and
//        the placing pass writes every entry straight to its slot.  No global atomics anywhere, so the layout
//        is a pure function of the matrix.
//
// HBM traffic per slot: 6 B read (5.75 with packed columns) + 4 B written in phase 1, 5 B read in phase 2 (15 B vs CSR's 8 B per entry) —
// but all of it is streamed, which beats one 64-byte random fetch per entry by a wide margin once x leaves L2.
// Reproducibility: layout and long-row sums are order-free; inside a tile the products of a row meet in
// scheduling order, but they are added as doubles (every fp32 product is exact there, the sum of a row's
// products carries ~29 spare bits) and rounded to fp32 once, so two runs give the same bits
// (tests/test_gpu_spmv.py holds this on C4 and C5 shapes).
//
// This file holds what an SpMV or a PageRank step executes: the two phases' kernels and their launchers.  The plan
// builder is tiled_cells.hip (ranking, placing, scans, pass layout) and tiled_build.hip (long rows, fold probe, phase-1
// items), the shape rules are tiled_plan.cpp; what builder and kernels must agree on is tiled_layout.h.
#include "tiled.h"
#include "tiled_layout.h"
#include "device_common.h"
#include "pagerank_engine.h"
#include "pr_commit_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// The products are written once and read once, by other CUs, a whole kernel later: stored NON-TEMPORAL they do not linger
// as dirty lines in the Infinity Cache, whose write-back would otherwise compete with phase 2's reads (phase 1 takes
// ~13 us longer on C5, phase 2 ~29 us less: 518 -> 509 us per SpMV same box, 512 -> 489 on another;
// profiles/r04_store_flavours.txt — sc1 / sc0 sc1 write-through stores and nt LOADS on either phase lose).
template <typename T>
__device__ __forceinline__ void store_product(T* p, T v) { __builtin_nontemporal_store(v, p); }

// ------------------------------------------------------------------------ phase 1 ----
// Rows too long for the cells are cut into chunks of kLongChunk entries; one wavefront per
// chunk sums it by direct gather into its own slot; phase 2's tile start then adds a long row's chunk sums in
// chunk order (no atomics, no state between calls: the same bits on every run).  The chunk wavefronts ride in
// extra workgroups at the head of the phase-1 grid, so they overlap the expansion at no launch cost.
struct LongRows {
    const int* chunks;        // (row, begin, end) triples over the CSR arrays
    int num_chunks;
    long long nnz;
    const int* cols;
    const float* vals;
    float* chunk_sum;         // [num_chunks] one partial sum per chunk (no atomics: long_rows_finish_kernel adds them in order)
};

__device__ __forceinline__ void long_row_chunk(const LongRows& lr, int which, const float* __restrict__ x) {
    if (which >= lr.num_chunks) return;
    float acc = row_partial_dot<64>(lr.chunks[3 * which + 1], lr.chunks[3 * which + 2], threadIdx.x & 63, lr.nnz,
                                    lr.cols, lr.vals, x);
    acc = group_sum<64>(acc);
    if ((threadIdx.x & 63) == 0) lr.chunk_sum[which] = acc;
}

// Stages x strip `strip` (W columns from `base`) into xs.  FOLD: as w_j * x_j (one rounded product per column).
// Whole rounds of the workgroup first, several 16-byte loads per lane in flight.  One load per iteration behind its own wait
// made a W = 16384 strip eight L2 latencies per item, ~20 % of a workgroup's life during which it streams nothing: C5
// phase 1 322-328 -> 310-312 us with four in flight (two: 313-317; eight, or the entry loop software-pipelined on top:
// no further change — profiles/r04_kernel_ab_descriptors.txt).
template <int W, int kExpandBlock, bool FOLD>
__device__ __forceinline__ void stage_strip(float* xs, const float* __restrict__ x, const float* __restrict__ col_weight,
                                            long long base, int num_cols) {
    const int width = static_cast<int>(min(static_cast<long long>(W), num_cols - base));
    const float* src = x + base;
    constexpr int kRound = kExpandBlock * 4;
    constexpr int kInFlight = W / kRound >= 4 ? 4 : (W / kRound >= 2 ? 2 : 1);
    if (FOLD) {
        const float* wsrc = col_weight + base;            // hipMalloc'd and base % 4 == 0: always aligned
        const bool aligned = (reinterpret_cast<unsigned long long>(src) & 15) == 0;
        int i_block = 0;                                   // wave-uniform
        if (aligned) {
#pragma unroll 1
            for (; i_block + kInFlight * kRound <= width; i_block += kInFlight * kRound) {
                const int i = i_block + threadIdx.x * 4;
                f32x4 xv[kInFlight], wv[kInFlight];
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    xv[u] = *reinterpret_cast<const f32x4*>(src + i + u * kRound);
                    wv[u] = *reinterpret_cast<const f32x4*>(wsrc + i + u * kRound);
                }
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    f32x4 z;
                    z[0] = __fmul_rn(wv[u][0], xv[u][0]);
                    z[1] = __fmul_rn(wv[u][1], xv[u][1]);
                    z[2] = __fmul_rn(wv[u][2], xv[u][2]);
                    z[3] = __fmul_rn(wv[u][3], xv[u][3]);
                    *reinterpret_cast<f32x4*>(xs + i + u * kRound) = z;
                }
            }
        }
        for (int i = i_block + threadIdx.x * 4; i < width; i += kRound) {
            if (aligned && i + 3 < width) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(src + i);
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wsrc + i);
                f32x4 z;
                z[0] = __fmul_rn(wv[0], xv[0]);
                z[1] = __fmul_rn(wv[1], xv[1]);
                z[2] = __fmul_rn(wv[2], xv[2]);
                z[3] = __fmul_rn(wv[3], xv[3]);
                *reinterpret_cast<f32x4*>(xs + i) = z;
            } else {
                for (int k = i; k < min(i + 4, width); ++k) xs[k] = __fmul_rn(wsrc[k], src[k]);
            }
        }
    } else if ((reinterpret_cast<unsigned long long>(src) & 15) == 0) {
        int i_block = 0;                                   // wave-uniform
#pragma unroll 1
        for (; i_block + kInFlight * kRound <= width; i_block += kInFlight * kRound) {
            const int i = i_block + threadIdx.x * 4;
            f32x4 t[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) t[u] = *reinterpret_cast<const f32x4*>(src + i + u * kRound);
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) *reinterpret_cast<f32x4*>(xs + i + u * kRound) = t[u];
        }
        for (int i = i_block + threadIdx.x * 4; i < width; i += kRound) {
            if (i + 3 < width) {
                *reinterpret_cast<f32x4*>(xs + i) = *reinterpret_cast<const f32x4*>(src + i);
            } else {
                for (int k = i; k < width; ++k) xs[k] = src[k];
            }
        }
    } else {
        for (int i = threadIdx.x; i < width; i += kExpandBlock) xs[i] = src[i];
    }
}

// The local columns of the four slots q .. q + 3 of a plan with PACKED columns (tiled_layout.h: 14 bits a slot, 256 slots
// in a 448-byte block): one aligned dword of the block's low plane and the 24 bits of its high field that start at byte
// 3 * lane — the wavefront walks one block per iteration, so the lane's group is group `lane` of the block.
struct Cols14 {
    unsigned int lo, hi;
    __device__ __forceinline__ int at(int e) const { return static_cast<int>(((lo >> (8 * e)) & 0xFFu) | (((hi >> (6 * e)) & 0x3Fu) << 8)); }
};
// The high bits: one 4-byte load at a byte address (a single global_load_dword; gfx950 takes the unaligned address), whose
// top byte is the next lane's, or the slack behind the array.  (The other form — 48 lanes load the field's aligned
// dwords, two ds_bpermute and a v_alignbyte hand every lane its 24 bits — made the kernel 30 to 34 us SLOWER than the
// u16 plan on C5, where this one is faster: the permutes queue behind the LDS gathers.  profiles/packed_cols_ab.txt.)
__device__ __forceinline__ unsigned int cols14_high(const unsigned char* __restrict__ block, int lane) {
    unsigned int hi;
    __builtin_memcpy(&hi, block + kColLowBytes + 3 * lane, sizeof(hi));
    return hi;
}

// The products of the slots [begin, end) of the staged strip: value, local column -> value * xs[column], same order.
// PACKED: a_cols is the plan's a_cols14, else its a_lcol (u16 per slot).
template <int kExpandBlock, bool FOLD, bool PACKED>
__device__ __forceinline__ void expand_slots(const float* xs, int begin, int end, const float* __restrict__ a_val,
                                             const void* __restrict__ a_cols, float* __restrict__ prod) {
    constexpr int kStride = kExpandBlock * 4;
    const unsigned short* __restrict__ a_lcol = PACKED ? nullptr : static_cast<const unsigned short*>(a_cols);
    const unsigned char* __restrict__ cols14 = PACKED ? static_cast<const unsigned char*>(a_cols) : nullptr;
    // Both loops start at the 16-slot boundary at or below `begin` (16 products = one 64-byte sector): a wavefront's 1 KB
    // of non-temporal stores then covers whole sectors, where an origin of begin & ~3 split a sector between two
    // instructions and, as such stores do not merge, wrote it twice (profiles/aligned_streams_traffic_ab.txt).  The
    // groups in front of `begin` are masked like those behind `end`: same products to the same slots.
    if (PACKED) {
        // The same walk from the 256-slot boundary at or below `begin`: kStride is a multiple of 256, so the 256 slots of a
        // wavefront's iteration are exactly one column block.  The loop runs on the wavefront's first slot, a scalar, and
        // so does the block's address; the groups outside [begin, end) are masked as above.  FOLD takes two groups a
        // workgroup-stride apart per step, as below.
        static_assert(kStride % kColBlockSlots == 0, "a wavefront's 256 slots are one column block");
        constexpr int kGroups = FOLD ? 2 : 1;
        const int lane = threadIdx.x & 63;
        const int wave_first = __builtin_amdgcn_readfirstlane((begin & ~(kColBlockSlots - 1)) + (static_cast<int>(threadIdx.x) - lane) * 4);
        for (int w = wave_first; w < end; w += kGroups * kStride) {
#pragma unroll
            for (int u = 0; u < kGroups; ++u) {
                const int first = w + u * kStride;
                if (first >= end) break;
                const unsigned char* block = cols14 + col_block_byte(first);
                const int q = first + 4 * lane;
                if (q >= begin && q + 3 < end) {
                    Cols14 c;
                    c.lo = reinterpret_cast<const unsigned int*>(block)[lane];
                    c.hi = cols14_high(block, lane);
                    f32x4 p;
                    if (FOLD) {
                        p[0] = xs[c.at(0)]; p[1] = xs[c.at(1)]; p[2] = xs[c.at(2)]; p[3] = xs[c.at(3)];
                    } else {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(a_val + q);
                        p[0] = v[0] * xs[c.at(0)];
                        p[1] = v[1] * xs[c.at(1)];
                        p[2] = v[2] * xs[c.at(2)];
                        p[3] = v[3] * xs[c.at(3)];
                    }
                    store_product(reinterpret_cast<f32x4*>(prod + q), p);
                } else {
                    for (int k = max(q, begin); k < min(q + 4, end); ++k) {
                        const float xk = xs[lcol_at(a_lcol, cols14, k)];
                        prod[k] = FOLD ? xk : a_val[k] * xk;
                    }
                }
            }
        }
        return;
    }
    if (FOLD) {
        // four entries per lane per group, two groups a workgroup-stride apart per step: every store instruction writes
        // one contiguous KB per wavefront (round 3's eight consecutive entries per lane made each instruction write every
        // other 16 bytes; harmless with plain stores, which meet in L2, but 31 % more write traffic with the non-temporal
        // ones: WRITE_SIZE 826 against 631 MB on C5)
        for (int q = (begin & ~15) + threadIdx.x * 4; q < end; q += 2 * kStride) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int g = q + u * kStride;
                if (g >= begin && g + 3 < end) {
                    const u16x4 c = *reinterpret_cast<const u16x4*>(a_lcol + g);
                    f32x4 p;
                    p[0] = xs[c[0]]; p[1] = xs[c[1]]; p[2] = xs[c[2]]; p[3] = xs[c[3]];
                    store_product(reinterpret_cast<f32x4*>(prod + g), p);
                } else {
                    for (int k = max(g, begin); k < min(g + 4, end); ++k) prod[k] = xs[lcol_at(a_lcol, cols14, k)];
                }
            }
        }
        return;
    }
    // four entries per lane per step, groups aligned to 4 entries (16-byte loads and stores).  (Round 4 tried 2 / 4 / 8 groups
    // per lane with all loads issued up front, and the next group's loads in flight while this one is multiplied: no gain,
    // the bunched forms lose 1-2 % — profiles/r04_kernel_ab_descriptors.txt; once a workgroup streams, phase 1 runs at the
    // rate its 10 bytes per slot allow.  What paid was the start of a workgroup's life: the staging.)
    for (int q = (begin & ~15) + threadIdx.x * 4; q < end; q += kStride) {
        if (q >= begin && q + 3 < end) {
            const u16x4 c = *reinterpret_cast<const u16x4*>(a_lcol + q);
            const f32x4 v = *reinterpret_cast<const f32x4*>(a_val + q);
            f32x4 p;
            p[0] = v[0] * xs[c[0]];
            p[1] = v[1] * xs[c[1]];
            p[2] = v[2] * xs[c[2]];
            p[3] = v[3] * xs[c[3]];
            store_product(reinterpret_cast<f32x4*>(prod + q), p);
        } else {
            for (int k = max(q, begin); k < min(q + 4, end); ++k) prod[k] = a_val[k] * xs[lcol_at(a_lcol, cols14, k)];
        }
    }
}

// FOLD: the plan holds one weight per column instead of a value per entry; the strip is staged
// as w_j * x_j and an entry's product is a plain LDS read (the same rounded product as a_ij * x_j).
// One workgroup per work item.  (Round 4 tried 2 / 3 / 5 CONSECUTIVE items per workgroup, staging a strip only when it changes:
// 347 / 359 / 433 against 320 us on C5 — fewer, longer workgroups balance worse than their saved strip loads are worth.)
// PACKED: the plan's local columns are the 14-bit blocks of tiled_layout.h (a_cols = a_cols14), else u16 per slot (a_lcol).
template <int W, int kExpandBlock, bool FOLD, bool PACKED>
__global__ __launch_bounds__(kExpandBlock)
void tiled_expand_kernel(const int* __restrict__ items, int first_item, int num_items, int commit_blocks, int long_blocks,
                         const float* __restrict__ a_val,
                         const void* __restrict__ a_cols,
                         const float* __restrict__ col_weight,
                         const float* __restrict__ x, int num_cols,
                         float* __restrict__ prod, LongRows long_rows,
                         const PrState* __restrict__ state, CommitRider commit) {
    // The previous step's residual commit, when it was deferred into this launch: workgroup 0 of a head of
    // commit_blocks (0 or 8, so that the XCD mapping below holds) folds that step's block partials into the state —
    // the arithmetic of pr_reduce_commit_kernel, on its first kBlock threads.  The partials were written by the
    // previous phase-2 launch, so the kernel boundary has made them visible to every XCD.
    if (static_cast<int>(blockIdx.x) < commit_blocks) {
        if (blockIdx.x == 0 && threadIdx.x < kBlock) pr_fold_and_commit(commit.partials, commit.num_blocks, commit.tolerance, commit.state);
        return;
    }
    // PageRank steps enqueued past convergence are no-ops.  `done` is read once per workgroup, and the commit
    // workgroup above may set it before or after that read.  Either order gives the same result: this launch
    // writes scratch only (products, long-row chunk sums), which nothing reads after `done` is set — this
    // step's phase 2 starts after this launch has completed, sees `done` and returns, as does every later step.
    // (The item record requested together with `done`, one scalar wait for both instead of one behind the other: the
    // kernel +0.3 +- 0.8 us on C5 over 28 interleaved pairs, nothing — profiles/step_ends_ab.txt.)
    if (state && state->done) return;
    const int head_blocks = commit_blocks + long_blocks;
    if (static_cast<int>(blockIdx.x) < head_blocks) {     // the long-row workgroups go first (latency-bound)
        constexpr int kPerBlock = kExpandBlock / 64;
        long_row_chunk(long_rows, (blockIdx.x - commit_blocks) * kPerBlock + (threadIdx.x >> 6), x);
        return;
    }
    __shared__ float xs[W];
    const int window = xcd_contiguous(blockIdx.x - head_blocks, num_items);   // head_blocks is a multiple of 8
    if (window < 0) return;
    const int item = first_item + window;
    const int strip = items[3 * item];
    const int begin = items[3 * item + 1];
    const int end = items[3 * item + 2];
    stage_strip<W, kExpandBlock, FOLD>(xs, x, col_weight, static_cast<long long>(strip) * W, num_cols);
    __syncthreads();
    expand_slots<kExpandBlock, FOLD, PACKED>(xs, begin, end, a_val, a_cols, prod);
}

// ------------------------------------------------------------------------ phase 2 ----
// the long rows (direct path): which of them fall into which tile, and where their chunk sums are
struct LongSeeds {
    const int* rows;          // [num_long] ascending
    const int* first_chunk;   // [num_long + 1]
    const int* tile_first;    // [num_tiles + 1] first long row of every tile (null: no long rows)
    const float* chunk_sum;   // [num_chunks] written by phase 1 of this SpMV
};

// Fills the LDS tile with the sums of this tile's rows; the long rows' sums come from their chunk sums.  The tile
// accumulates in DOUBLE: every fp32 product is added exactly as often as fp64 allows (products of one row rarely span
// more than 29 binades), so the row sums do not depend on the order in which the wavefronts' adds meet, and they are
// rounded to fp32 once, on the way out.
// In two pieces, tile_seed and tile_stream, so that the PageRank form can ask for the wavefront's pass range before the
// first of them (the start of a tile's life, below); tile_accumulate is both, as the plain reduce runs them.
__device__ __forceinline__ void tile_seed(double* tile, int R, int tile_index, const LongSeeds seeds) {
    const long long first = static_cast<long long>(tile_index) * R;
    for (int i = threadIdx.x; i < R; i += kReduceThreads) tile[i] = 0.0;
    if (seeds.tile_first) {
        __syncthreads();
        for (int k = seeds.tile_first[tile_index] + threadIdx.x; k < seeds.tile_first[tile_index + 1]; k += kReduceThreads) {
            double total = 0.0;                         // a long row's chunk sums, in chunk order
            for (int c = seeds.first_chunk[k]; c < seeds.first_chunk[k + 1]; ++c) total += static_cast<double>(seeds.chunk_sum[c]);
            tile[seeds.rows[k] - first] = total;
        }
    }
    __syncthreads();
}

// The calling wavefront's passes [pass_lo, pass_hi) added into the seeded tile, and the barrier that closes the tile.
__device__ __forceinline__ void tile_stream(double* tile, int pass_lo, int pass_hi, const PassDesc* __restrict__ desc,
                                            const float* __restrict__ prod,
                                            const unsigned int* __restrict__ pass_word) {
    __shared__ double spare[64];           // where a lane's slots without an entry "add" (never read)
    const int lane = threadIdx.x & 63;

    struct Pass {
        int lane_adj;                      // adj of the lane's segment (selected when the pass is opened: a select over struct
        f32x4 p;                           //  members kept for later turns into an indexed load from scratch memory)
        unsigned int d;                    // the lane's four row deltas; all kSkip on the lanes past the pass's end
    };
    // descriptors 64 at a time: lane l holds pass window_first + l
    for (int window_first = pass_lo; window_first < pass_hi; window_first += 64) {
        const uint4* mine = reinterpret_cast<const uint4*>(desc + window_first + min(lane, pass_hi - window_first - 1));
        uint4 lo = mine[0], hi = mine[1];
        // (waited for HERE, once: read for the first time inside the loop below, the compiler would wait vmcnt(0) — the
        // passes' own loads included — at every pass it opens)
        asm volatile("; pass descriptors settled" : "+v"(lo.x), "+v"(lo.y), "+v"(lo.z), "+v"(lo.w), "+v"(hi.x), "+v"(hi.y), "+v"(hi.z));
        const int window_passes = min(64, pass_hi - window_first);

        auto open = [&](Pass& ps, int k) {            // pass k of the window (k < window_passes): geometry + its two loads
            const int idx = __builtin_amdgcn_readfirstlane(k);
            const int base0 = __builtin_amdgcn_readlane(static_cast<int>(lo.x), idx);
            const int base1 = __builtin_amdgcn_readlane(static_cast<int>(lo.y), idx);
            const int base2 = __builtin_amdgcn_readlane(static_cast<int>(lo.z), idx);
            const int adj0 = __builtin_amdgcn_readlane(static_cast<int>(lo.w), idx);
            const int adj1 = __builtin_amdgcn_readlane(static_cast<int>(hi.x), idx);
            const int adj2 = __builtin_amdgcn_readlane(static_cast<int>(hi.y), idx);
            const unsigned int geom = static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(hi.z), idx));
            const int start1 = static_cast<int>(geom & 0xFF), start2 = static_cast<int>((geom >> 8) & 0xFF);
            const int groups = static_cast<int>(geom >> 16);
            // The row deltas come from the pass-ordered copy the builder laid out (pass_word, tiled_layout.h): one aligned
            // 256-byte block per pass, whatever the segments.  Lanes past the pass's end find four skip markers there;
            // their product load re-reads the pass's last group (same cache line).
            ps.d = pass_word[(static_cast<size_t>(window_first) + idx) * 64 + lane];
            const int at = min(lane, groups - 1);
            int base = base0, adj = adj0;
            base = at >= start1 ? base1 : base;
            adj = at >= start1 ? adj1 : adj;
            base = at >= start2 ? base2 : base;
            adj = at >= start2 ? adj2 : adj;
            ps.lane_adj = adj;
            const unsigned int slot = static_cast<unsigned int>(base + 4 * at);
            ps.p = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(prod) + (static_cast<size_t>(slot) << 2));
        };
        auto add = [&](const Pass& ps) {
            const unsigned int word = ps.d;
            int delta[4], upto[4], sum = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                delta[e] = (word >> (8 * e)) & 0xFF;
                sum += delta[e];
                upto[e] = sum;
            }
            const int incl = wave_inclusive_scan(sum);
            const int lane_base = ps.lane_adj + incl - sum;
            // One LDS atomic per slot: ds_add_f64 (no return value, no retry loop, equal rows in one instruction are the
            // hardware's business; gfx950 runs it at 3.5 lanes/clk/CU on random rows, the fp32 form at 0.38 —
            // tools/lds_bench.hip).  Skip markers aim at a per-lane spare word, so nothing here needs an execution mask.
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double* target = delta[e] != kSkip ? &tile[lane_base + upto[e]] : &spare[lane];
                atomicAdd(target, static_cast<double>(ps.p[e]));
            }
        };

        // kPassDepth passes in flight, pass i of the window in slot i mod kPassDepth.  The steady-state loop holds nothing
        // but the pipeline (every add is followed by an open: no branch around a load, so the compiler's s_waitcnt in front
        // of an add counts exactly the newer passes' loads); what is left at the end is drained by the two short tails.
        Pass ps[kPassDepth];
#pragma unroll
        for (int u = 0; u < kPassDepth; ++u) {
            // (unconditional — a window shorter than the pipeline re-opens its last pass and never adds it —: with branches
            // here the loads in flight differ from path to path and the first wait of the loop below becomes vmcnt(0))
            open(ps[u], min(u, window_passes - 1));
            __builtin_amdgcn_sched_barrier(0);
        }
        int k = 0;
        for (; k + 2 * kPassDepth <= window_passes; k += kPassDepth) {
#pragma unroll
            for (int u = 0; u < kPassDepth; ++u) {
                // (scheduling barriers: left alone, the compiler gathers the three adds behind ONE s_waitcnt vmcnt(0) and issues
                // all six loads at the end of the iteration — nothing in flight while a pass is added)
                add(ps[u]);
                __builtin_amdgcn_sched_barrier(0);
                open(ps[u], k + u + kPassDepth);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int u = 0; u < kPassDepth; ++u) {
            if (k + u < window_passes) {
                add(ps[u]);
                if (k + u + kPassDepth < window_passes) open(ps[u], k + u + kPassDepth);
            }
        }
#pragma unroll
        for (int u = 0; u < kPassDepth; ++u) {
            if (k + kPassDepth + u < window_passes) add(ps[u]);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void tile_accumulate(double* tile, int R, int tile_index,
                                                const int* __restrict__ pass_first, const PassDesc* __restrict__ desc,
                                                const float* __restrict__ prod,
                                                const unsigned int* __restrict__ pass_word,
                                                const LongSeeds seeds) {
    tile_seed(tile, R, tile_index, seeds);
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int pass_lo = pass_first[tile_index * kReduceWaves + wave], pass_hi = pass_first[tile_index * kReduceWaves + wave + 1];
    tile_stream(tile, pass_lo, pass_hi, desc, prod, pass_word);
}

// The tile (R doubles, R = plan.tile_rows: any multiple of 64) lives in dynamic LDS.
template <int kReduceBlock>
__global__ __launch_bounds__(kReduceBlock, kReduceBlock / 128)     // two tiles per CU: 8 wavefronts per SIMD
void tiled_reduce_kernel(int R, int num_tiles, const int* __restrict__ pass_first, const PassDesc* __restrict__ pass_desc,
                         const float* __restrict__ prod,
                         const unsigned int* __restrict__ pass_word,
                         const LongSeeds seeds,
                         int num_rows, float* __restrict__ y) {
    static_assert(kReduceBlock == kReduceThreads, "the pass layout is made for this workgroup size");
    extern __shared__ double tile[];
    const int tile_index = xcd_contiguous(blockIdx.x, num_tiles);
    if (tile_index < 0) return;
    tile_accumulate(tile, R, tile_index, pass_first, pass_desc, prod, pass_word, seeds);
    const long long first = static_cast<long long>(tile_index) * R;
    for (int i = threadIdx.x; i < R && first + i < num_rows; i += kReduceBlock) y[first + i] = static_cast<float>(tile[i]);
}

// phase 2 with the PageRank update fused into the tile write-out (cf. pr_step_kernel)
template <int kReduceBlock>
__global__ __launch_bounds__(kReduceBlock, kReduceBlock / 128)
void tiled_pagerank_reduce_kernel(int R, int num_tiles, const int* __restrict__ pass_first, const PassDesc* __restrict__ pass_desc,
                                  const float* __restrict__ prod,
                                  const unsigned int* __restrict__ pass_word,
                                  const LongSeeds seeds,
                                  int local_rows, RowMap map, int n_global,
                                  const float* __restrict__ r_old, float* __restrict__ r_new,
                                  const unsigned char* __restrict__ dangling, DanglingBits bits, float damping,
                                  const PrState* __restrict__ state,
                                  double* __restrict__ block_partials, PushTargets push) {
    extern __shared__ double tile[];
    const int tile_index = xcd_contiguous(blockIdx.x, num_tiles);
    if (tile_index < 0) return;
    // The start of a tile's life.  Everything it reads through the scalar path is asked for here, together, and waited
    // for once: `done`, the dangling mass (on the same line; first read behind the tile's closing barrier it was one more
    // exposed latency there), the tile's flagged-row count and the wavefront's pass range (first read behind the cleared
    // tile's barrier).  Read one behind the other they were four dependent waits per tile, and a uniform matrix brings all
    // 512 resident workgroups to them together: moments at which the whole chip streams nothing.  C5's step kernel
    // 0.7 us shorter by itself, 1.1 us on top of the non-temporal r_new stores below (profiles/step_ends_ab.txt).
    // Without flag words the count's load reads `done` again: no branch around a load.
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int* range = pass_first + tile_index * kReduceWaves + wave;
    const int* count_word = bits.words ? bits.tile_count + tile_index : &state->done;
    int done = state->done, mass_bits = __float_as_int(state->dangling_sum), pass_lo = range[0], pass_hi = range[1];
    int flagged = *count_word;
    asm volatile("; tile head settled" : "+s"(done), "+s"(mass_bits), "+s"(pass_lo), "+s"(pass_hi), "+s"(flagged));
    if (done) return;
    const int flagged_rows = bits.words ? flagged : 0;
    tile_seed(tile, R, tile_index, seeds);
    tile_stream(tile, pass_lo, pass_hi, pass_desc, prod, pass_word);

    const float teleport = __fdiv_rn(1.0f - damping, static_cast<float>(n_global));
    const float dangling_term = __fdiv_rn(__fmul_rn(damping, __int_as_float(mass_bits)),
                                          static_cast<float>(n_global));
    double res2 = 0.0, mass = 0.0;
    const long long first = static_cast<long long>(tile_index) * R;
    if (map.piece == 0x7fffffff && push.count == 0) {
        // The usual case (one contiguous slice, no peer stores).  The update needs r_old and the dangling flag of the tile's
        // rows: read inside the loop they were one full memory latency per row and thread, ten in a row (the loop below waits
        // vmcnt(0) in every iteration: +22 us per step on C5, 182 against 160 us for the plain reduce); here all of a
        // thread's loads go out together, in front of the arithmetic.  Same operations in the same order: same bits.
        // (Issued one step earlier still, behind a wavefront's last add and in front of the tile's closing barrier, so that
        // they fly while the slower wavefronts drain: +0.1 +- 0.16 us by itself, -0.5 +- 0.3 on top of what is here now —
        // nothing to tell from the noise, profiles/step_ends_ab.txt.)
        constexpr int kPerThread = (kMaxTileRows + kReduceBlock - 1) / kReduceBlock;
        const long long node_first = map.base + first;
        const int rows_here = static_cast<int>(min(static_cast<long long>(R), local_rows - first));     // >= 1: the tile exists
        float old_rank[kPerThread];
        unsigned int is_dangling[kPerThread];
        // (unconditional loads at clamped rows: a guarded load is a branch, and the compiler waits for each behind its join)
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) {
            const int i = min(static_cast<int>(threadIdx.x) + u * kReduceBlock, rows_here - 1);
            old_rank[u] = r_old[node_first + i];
        }
        // The flags: one BIT per local row where the shard holds them (DanglingBits, pagerank_engine.h) — a wavefront reads
        // the two words of its 64 rows instead of 64 bytes — and nothing at all for a tile without a dangling row, which
        // in a web graph is most of them.  One wave-uniform branch around all of a thread's flag loads, none around each;
        // the loads only load (the word is kept, its bit is taken below: a shift right behind each load made the compiler
        // wait for every word before it asked for the next).  A tile starts on a multiple of 64 rows and the threads of a
        // round are 1024 rows apart, so the bit of row i of the tile is bit threadIdx.x % 32 of its word in every round.
        const bool packed = bits.words != nullptr;
        const unsigned int flag_shift = packed ? threadIdx.x & 31u : 0u;
        if (!packed) {
#pragma unroll
            for (int u = 0; u < kPerThread; ++u) {
                const int i = min(static_cast<int>(threadIdx.x) + u * kReduceBlock, rows_here - 1);
                is_dangling[u] = dangling[node_first + i];
            }
        } else if (flagged_rows != 0) {
#pragma unroll
            for (int u = 0; u < kPerThread; ++u) {
                const long long row = first + min(static_cast<int>(threadIdx.x) + u * kReduceBlock, rows_here - 1);
                is_dangling[u] = bits.words[row >> 5];
            }
        } else {
#pragma unroll
            for (int u = 0; u < kPerThread; ++u) is_dangling[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < kPerThread; ++u) {
            const int i = threadIdx.x + u * kReduceBlock;
            if (i < rows_here) {
                const float fresh = __fadd_rn(__fadd_rn(__fmul_rn(damping, static_cast<float>(tile[i])), dangling_term), teleport);
                // Non-temporal, like the products: nothing reads r_new through this XCD's L2 before the next launch, and
                // stored plain a round's tiles leave ~20 MB of dirty lines there for the kernel's end to write back
                // (C5: the kernel 3.1 us shorter, phase 1 of the next step — which reads the vector — unchanged).
                __builtin_nontemporal_store(fresh, &r_new[node_first + i]);
                const float diff = __fsub_rn(fresh, old_rank[u]);
                res2 += static_cast<double>(__fmul_rn(diff, diff));
                if (packed ? (is_dangling[u] >> flag_shift) & 1u : is_dangling[u]) mass += static_cast<double>(fresh);
            }
        }
    } else {
        for (int i = threadIdx.x; i < R && first + i < local_rows; i += kReduceBlock) {
            const long long node = map.at(first + i);
            const float fresh = __fadd_rn(__fadd_rn(__fmul_rn(damping, static_cast<float>(tile[i])), dangling_term), teleport);
            r_new[node] = fresh;
            for (int p = 0; p < push.count; ++p) push.ptr[p][node] = fresh;     // straight into the peers' vectors
            const float diff = __fsub_rn(fresh, r_old[node]);
            res2 += static_cast<double>(__fmul_rn(diff, diff));
            if (dangling[node]) mass += static_cast<double>(fresh);
        }
    }
    block_sum2<kReduceBlock>(res2, mass);
    if (threadIdx.x == 0) {
        block_partials[2 * tile_index] = res2;
        block_partials[2 * tile_index + 1] = mass;
    }
}

// the product stream and the long-row chunk sums a call on stream `s` writes (see TiledPlan::StreamScratch)
struct Scratch {
    float* prod;
    float* long_sums;
};
constexpr size_t kMaxExtraScratch = 7;

hipError_t scratch_for(const TiledPlan& plan, hipStream_t s, Scratch* out) {
    std::lock_guard<std::mutex> guard(plan.scratch_lock);
    if (!plan.primary_taken) {
        plan.primary_taken = true;
        plan.primary_stream = s;
    }
    if (plan.primary_stream == s) {
        *out = Scratch{plan.prod.get(), plan.long_sums.get()};
        return hipSuccess;
    }
    for (const TiledPlan::StreamScratch& e : plan.extra_scratch) {
        if (e.stream == s) {
            *out = Scratch{e.prod.get(), e.long_sums.get()};
            return hipSuccess;
        }
    }
    if (plan.extra_scratch.size() >= kMaxExtraScratch) return hipErrorOutOfMemory;
    auto floats = [](DevBuf<float>* buf, long long count) {
        float* p = nullptr;
        const hipError_t e = malloc_any_time(reinterpret_cast<void**>(&p), static_cast<size_t>(count) * sizeof(float));
        buf->reset(e == hipSuccess ? p : nullptr);
        return e;
    };
    TiledPlan::StreamScratch fresh;
    fresh.stream = s;
    if (floats(&fresh.prod, plan.nnz + 8) != hipSuccess || floats(&fresh.long_sums, std::max(plan.num_long_chunks, 1)) != hipSuccess) {
        (void)hipGetLastError();
        return hipErrorOutOfMemory;
    }
    *out = Scratch{fresh.prod.get(), fresh.long_sums.get()};
    plan.extra_scratch.push_back(std::move(fresh));
    return hipSuccess;
}

// phase 1 for the items [first_item, first_item + num_items) and, with_long, the long-row chunks
template <int W, int BLOCK>
hipError_t launch_expand_as(const TiledPlan& plan, const Scratch& sc, int first_item, int num_items, bool with_long,
                            const float* d_x, const PrState* d_state, const CommitRider& commit, hipStream_t s) {
    const int chunks = with_long ? plan.num_long_chunks : 0;
    const LongRows lr{plan.long_chunks.get(), chunks, plan.csr_nnz, plan.csr_cols, plan.csr_vals, sc.long_sums};
    const int long_blocks = xcd_grid((chunks + BLOCK / 64 - 1) / (BLOCK / 64));
    const int commit_blocks = commit.partials ? kXcds : 0;
    const int grid = commit_blocks + long_blocks + xcd_grid(num_items);
    if (grid == 0) return hipSuccess;
    auto launch = [&](auto fold, auto packed) {
        constexpr bool FOLD = decltype(fold)::value, PACKED = decltype(packed)::value;
        const void* cols = PACKED ? static_cast<const void*>(plan.a_cols14.get()) : static_cast<const void*>(plan.a_lcol.get());
        tiled_expand_kernel<W, BLOCK, FOLD, PACKED><<<grid, BLOCK, 0, s>>>(
            plan.items.get(), first_item, num_items, commit_blocks, long_blocks, plan.a_val.get(), cols, plan.col_weight.get(), d_x,
            plan.num_cols, sc.prod, lr, d_state, commit);
    };
    // (a 32768-column strip never packs: no such instantiation)
    const bool packed = W <= kPackedStripCols && plan.a_cols14 != nullptr;
    if (plan.col_weight) {
        if (packed) launch(std::true_type{}, std::integral_constant<bool, (W <= kPackedStripCols)>{});
        else launch(std::true_type{}, std::false_type{});
    } else {
        if (packed) launch(std::false_type{}, std::integral_constant<bool, (W <= kPackedStripCols)>{});
        else launch(std::false_type{}, std::false_type{});
    }
    return hipGetLastError();
}

hipError_t launch_expand(const TiledPlan& plan, const Scratch& sc, int first_item, int num_items, bool with_long,
                         const float* d_x, const PrState* d_state, const CommitRider& commit, hipStream_t s) {
    return with_strip_width(plan.strip_cols, [&](auto width) {
        constexpr int W = decltype(width)::value;
        constexpr int BLOCK = W <= 16384 ? 512 : 1024;      // 32768 columns are 128 KiB of LDS: one workgroup per CU
        return launch_expand_as<W, BLOCK>(plan, sc, first_item, num_items, with_long, d_x, d_state, commit, s);
    });
}

LongSeeds long_seeds(const TiledPlan& plan, const Scratch& sc) {
    return LongSeeds{plan.long_rows.get(), plan.long_first.get(), plan.num_long > 0 ? plan.tile_long.get() : nullptr, sc.long_sums};
}

hipError_t launch_reduce(const TiledPlan& plan, const Scratch& sc, float* d_y, hipStream_t s) {
    const size_t lds = static_cast<size_t>(plan.tile_rows) * sizeof(double);
    const void* kernel = reinterpret_cast<const void*>(&tiled_reduce_kernel<kReduceThreads>);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    tiled_reduce_kernel<kReduceThreads><<<xcd_grid(plan.num_tiles), kReduceThreads, lds, s>>>(
        plan.tile_rows, plan.num_tiles, plan.pass_first.get(), plan.pass_desc.get(), sc.prod, plan.pass_word.get(),
        long_seeds(plan, sc), plan.num_rows, d_y);
    return hipGetLastError();
}

hipError_t launch_pagerank_reduce(const TiledPlan& plan, const Scratch& sc, const RowMap& map, int n_global, const float* d_r_old,
                                  float* d_r_new, const unsigned char* d_dangling, const DanglingBits& bits, float damping,
                                  const PrState* d_state, double* d_block_partials,
                                  const PushTargets& push, hipStream_t s) {
    const size_t lds = static_cast<size_t>(plan.tile_rows) * sizeof(double);
    const void* kernel = reinterpret_cast<const void*>(&tiled_pagerank_reduce_kernel<kReduceThreads>);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    tiled_pagerank_reduce_kernel<kReduceThreads><<<xcd_grid(plan.num_tiles), kReduceThreads, lds, s>>>(
        plan.tile_rows, plan.num_tiles, plan.pass_first.get(), plan.pass_desc.get(), sc.prod, plan.pass_word.get(),
        long_seeds(plan, sc), plan.num_rows, map, n_global, d_r_old, d_r_new, d_dangling, bits, damping, d_state,
        d_block_partials, push);
    return hipGetLastError();
}

} // namespace

hipError_t tiled_spmv(const TiledPlan& plan, const float* d_x, float* d_y, hipStream_t s) {
    Scratch sc;
    hipError_t e = scratch_for(plan, s, &sc);
    if (e != hipSuccess) return e;
    // two host threads may call on the same stream: the pair of launches must not interleave with another pair
    std::lock_guard<std::mutex> pair(plan.launch_lock);
    e = launch_expand(plan, sc, 0, plan.num_items, true, d_x, nullptr, CommitRider{}, s);       // phase 1 + the long rows
    if (e != hipSuccess) return e;
    return launch_reduce(plan, sc, d_y, s);
}

// After convergence the kernels of both parts return at once: r_new and the product stream stay as the last
// committed step left them.
hipError_t tiled_pagerank_expand(const TiledPlan& plan, int strip_begin, int strip_end, bool with_long,
                                 const float* d_r_old, const PrState* d_state, const CommitRider& commit, hipStream_t s) {
    Scratch sc;
    const hipError_t e = scratch_for(plan, s, &sc);
    if (e != hipSuccess) return e;
    strip_begin = std::max(0, std::min(strip_begin, plan.num_strips));
    strip_end = std::max(strip_begin, std::min(strip_end, plan.num_strips));
    const int first = plan.strip_first_item[strip_begin];
    return launch_expand(plan, sc, first, plan.strip_first_item[strip_end] - first, with_long, d_r_old, d_state, commit, s);
}

hipError_t tiled_pagerank_finish(const TiledPlan& plan, const RowMap& map, int n_global,
                                 const float* d_r_old, float* d_r_new,
                                 const unsigned char* d_dangling, const DanglingBits& bits, float damping,
                                 const PrState* d_state, double* d_block_partials,
                                 const PushTargets& push, hipStream_t s) {
    Scratch sc;
    const hipError_t e = scratch_for(plan, s, &sc);
    if (e != hipSuccess) return e;
    return launch_pagerank_reduce(plan, sc, map, n_global, d_r_old, d_r_new, d_dangling, bits, damping, d_state,
                                  d_block_partials, push, s);
}

} // namespace detail
} // namespace spmv

