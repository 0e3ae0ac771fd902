// tiled_cells.hip — first half of the LDS-tiled engine's plan builder (tiled.hip describes the engine and its layout):
// the entries of a CSR or ELL matrix are ranked and placed into the plan's cells, the cell table is scanned and phase 2's
// passes are laid out.  tiled_build.hip calls build_cells / layout_passes (tiled_build.h) and finishes the plan.
#include "tiled_build.h"
#include "tiled_layout.h"
#include "device_common.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

// ------------------------------------------------------------------ plan building ----
constexpr int kBuildBlock = 1024;           // threads of a builder workgroup
constexpr int kBuildRowCache = 1024;        // row offsets of the batch kept in LDS for the entry -> row search
constexpr int kBuildLdsSmall = 70 * 1024;   // dynamic LDS of a builder workgroup (two per CU, next to 8 KiB static) ...
constexpr int kBuildLdsLarge = 148 * 1024;  // ... or one per CU when the strips are many
constexpr int kBuildBinWords = 4;           // LDS ints per strip: start, cursor, markers, first|last
constexpr int kBuildEntryBytes = 11;        // LDS bytes per entry: key 4, source index 4 (the row marks, 2, live there first), bin 2, markers 1
// per strip, next to the four bin words: one byte per wavefront of the ranking workgroup (sixteen): the stable binning's counters
constexpr int kBuildWaveCountBytes = kBuildBlock / 64;

// where the entries come from.  offset(row) = index of the row's first entry in a virtual row-major
// numbering; col() < 0 marks ELL padding.
struct CsrSource {
    const int* row_ptrs;
    const int* cols;
    const float* vals;
    __device__ __forceinline__ long long offset(int row) const { return row_ptrs[row]; }
    __device__ __forceinline__ int col(long long j) const { return cols[j]; }
    __device__ __forceinline__ float val(long long j) const { return vals[j]; }
    static constexpr bool kSearchRows = true;      // an entry's row comes from a search over the row offsets
    __device__ __forceinline__ int direct_row(long long) const { return 0; }
};
struct EllSource {
    int rows, width;
    const int* cols;
    const float* vals;
    __device__ __forceinline__ long long offset(int row) const { return static_cast<long long>(row) * width; }
    __device__ __forceinline__ long long slot(long long j, int row) const {
        return (j - static_cast<long long>(row) * width) * rows + row;
    }
    static constexpr bool kSearchRows = false;     // rows have a fixed width
    __device__ __forceinline__ int direct_row(long long j) const { return static_cast<int>(j / width); }
    __device__ __forceinline__ int col(long long j) const { return cols[slot(j, direct_row(j))]; }
    __device__ __forceinline__ float val(long long j) const { return vals[slot(j, direct_row(j))]; }
};

struct BuildShape {
    int num_rows, num_tiles, num_strips, strip_shift, tile_rows, long_row;
    int any_long;               // some row is longer than long_row (then every entry's row length is checked)
    int stable_bins;            // the ranking pass may bin stably (no ranking loop); 0: always rank by comparison (SPMV_DEBUG=rank=plain)
    long long quota;            // entries per batch before the next one starts
};

// longest row (capped by the caller): sizes the batches
// one atomicMax per WORKGROUP: every wavefront adding its own to one address serialises 8 K atomics at the memory side (~80 us)
__device__ __forceinline__ void publish_block_max(int best, int* __restrict__ out) {
    __shared__ int s_best[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) best = max(best, __shfl_xor(best, off, 64));
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = s_best[0];
        for (int w = 1; w < kBlock / 64; ++w) all = max(all, s_best[w]);
        if (all > 0) atomicMax(out, all);
    }
}

template <typename Src>
__global__ __launch_bounds__(kBlock)
void max_row_kernel(Src src, int num_rows, int* __restrict__ out) {
    int best = 0;
    if constexpr (Src::kSearchRows) {
        // CSR: four rows per thread and step — one 16-byte load of the row pointers + the one behind them; a base off the
        // 16-byte boundary (a slice of a larger array) takes the plain loop below (tests/test_gpu_array_views.py)
        const int* rp = src.row_ptrs;
        if ((reinterpret_cast<unsigned long long>(rp) & 15) == 0) {
            const long long groups = num_rows / 4;
            for (long long g = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; g < groups;
                 g += static_cast<long long>(gridDim.x) * kBlock) {
                const i32x4 v = *reinterpret_cast<const i32x4*>(rp + 4 * g);
                const int next = rp[4 * g + 4];
                best = max(max(best, v[1] - v[0]), max(max(v[2] - v[1], v[3] - v[2]), next - v[3]));
            }
            if (blockIdx.x == 0 && threadIdx.x < num_rows % 4) {
                const int r = num_rows / 4 * 4 + threadIdx.x;
                best = max(best, rp[r + 1] - rp[r]);
            }
            publish_block_max(best, out);
            return;
        }
    }
    for (long long r = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; r < num_rows;
         r += static_cast<long long>(gridDim.x) * kBlock) {
        best = max(best, static_cast<int>(src.offset(static_cast<int>(r) + 1) - src.offset(static_cast<int>(r))));
    }
    publish_block_max(best, out);
}

// batches per tile: a tile's rows are cut wherever the running entry count passes a multiple of quota
template <typename Src>
__global__ __launch_bounds__(kBlock)
void tile_batches_kernel(Src src, BuildShape sh, int* __restrict__ count) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= sh.num_tiles) return;
    const int r0 = static_cast<int>(min(static_cast<long long>(t) * sh.tile_rows, static_cast<long long>(sh.num_rows)));
    const int r1 = static_cast<int>(min(static_cast<long long>(r0) + sh.tile_rows, static_cast<long long>(sh.num_rows)));
    const long long entries = src.offset(r1) - src.offset(r0);
    count[t] = static_cast<int>(max(1LL, (entries + sh.quota - 1) / sh.quota));
}

// first row of every batch (binary search for the batch's entry offset inside its tile)
template <typename Src>
__global__ __launch_bounds__(kBlock)
void batch_rows_kernel(Src src, BuildShape sh, const int* __restrict__ tile_batch /*[tiles + 1]*/,
                       int* __restrict__ batch_row /*[batches + 1]*/, int* __restrict__ batch_tile) {
    const int t = blockIdx.x;
    const int r0 = static_cast<int>(min(static_cast<long long>(t) * sh.tile_rows, static_cast<long long>(sh.num_rows)));
    const int r1 = static_cast<int>(min(static_cast<long long>(r0) + sh.tile_rows, static_cast<long long>(sh.num_rows)));
    const long long origin = src.offset(r0);
    const int first = tile_batch[t], n = tile_batch[t + 1] - first;
    for (int b = threadIdx.x; b < n; b += kBlock) {
        const long long target = origin + static_cast<long long>(b) * sh.quota;
        int lo = r0, hi = r1;                         // first row whose offset >= target
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (src.offset(mid) >= target) hi = mid; else lo = mid + 1;
        }
        batch_row[first + b] = lo;
        batch_tile[first + b] = t;
    }
    if (t == sh.num_tiles - 1 && threadIdx.x == 0) batch_row[tile_batch[sh.num_tiles]] = sh.num_rows;
}

// per (batch, strip) group: what the ranking pass learns / what the placing pass needs (same 8-byte slot)
struct GroupCount { unsigned short count, first, last, escapes; };      // escapes: markers in front of the non-first slots
struct GroupPlace { unsigned int rel; unsigned short prev_last, lead; };   // rel: offset inside the cell; lead: markers
                                                                         // in front of the group's first slot
static_assert(sizeof(GroupCount) == 8 && sizeof(GroupPlace) == 8, "group records share storage");

// Per-entry record the ranking pass leaves for the placing pass (indexed like the source entries):
//   the first slot of its group : 1 << 31 | row inside the tile   (its delta and markers depend on the cell's
//                                                                   earlier batches: cell_place_kernel settles them)
//   any other slot              : p << 16 | markers << 8 | delta   (p = slots of the group in front of it, its own
//                                                                   markers included, the group's lead excluded)
//   an entry of a long row      : kMetaSkip
constexpr unsigned int kMetaFirst = 1u << 31;
constexpr unsigned int kMetaSkip = 0xFFFFFFFFu;
constexpr int kBuildPerThread = 8;                     // entries a builder thread keeps in registers
constexpr int kBuildMaxCapacity = kBuildBlock * kBuildPerThread;

// Exclusive scan over the threads of a builder workgroup (1024 = 16 wavefronts) of one non-negative int each —
// a sum, or a running maximum.  Shuffles inside the wavefronts and 16 wavefront totals through LDS: two barriers
// where a Hillis-Steele ladder over an LDS array takes twenty (three such scans per batch were about half of a
// batch's time).  `scratch`: 16 ints of LDS; `*all` receives the total of the whole workgroup.
template <bool kMax>
__device__ __forceinline__ int block_exclusive_scan(int own, int* scratch, int* all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int other = __shfl_up(incl, off, 64);
        if (lane >= off) incl = kMax ? max(incl, other) : incl + other;
    }
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0) before = 0;
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    int prefix = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBuildBlock / 64; ++w) {
        const int t = scratch[w];
        if (w < wave) prefix = kMax ? max(prefix, t) : prefix + t;
        total = kMax ? max(total, t) : total + t;
    }
    __syncthreads();
    *all = total;
    return kMax ? max(prefix, before) : prefix + before;
}

// One batch (consecutive rows of one tile, at most `capacity` short-row entries): bin the entries by strip in
// LDS, rank every entry inside its bin by (row, column), derive the row deltas and the skip markers they need;
// report every bin's size and leave the per-entry records.  Dynamic LDS: kBuildBinWords ints per strip, then
// per entry key u32, source index u32, bin u16, row mark u16, markers u8.
template <typename Src>
__global__ __launch_bounds__(kBuildBlock, 8)          // two workgroups per CU: at most 64 registers
void batch_rank_kernel(Src src, BuildShape sh, int num_batches, int capacity,
                       const int* __restrict__ batch_row, const int* __restrict__ batch_tile,
                       uint2* __restrict__ groups,                 // [batches * strips] GroupCount
                       unsigned int* __restrict__ meta,            // [source entries]
                       int* __restrict__ long_rows, int* __restrict__ num_long) {
    extern __shared__ int build_lds[];
    __shared__ int s_partial[kBuildBlock / 64];
    __shared__ int s_row_cache[kBuildRowCache + 1];
    __shared__ int s_overflow;
    const int batch = xcd_contiguous(blockIdx.x, num_batches);
    if (batch < 0) return;
    const int S = sh.num_strips;
    int* bin_start = build_lds;                 // [S] first slot of the bin (after the scan)
    int* bin_cursor = build_lds + S;            // [S] histogram, then fill cursor (= bin end once filled)
    int* bin_escapes = build_lds + 2 * S;       // [S] skip markers needed in front of the bin's non-first slots
    int* bin_ends = build_lds + 3 * S;          // [S] first lrow << 16 | last lrow
    // per wavefront and strip one BYTE (four strips to a word): how many of the wavefront's entries fall into the strip,
    // then where in the bin its next one goes (stable binning, below)
    const int S4 = (S + 3) / 4;                 // words per wavefront
    unsigned int* wave_count = reinterpret_cast<unsigned int*>(build_lds + kBuildBinWords * S);
    unsigned int* keys = wave_count + (kBuildBlock / 64) * S4;    // lrow << 16 | lcol
    unsigned int* source = keys + capacity;     // index of the slot's entry, relative to the batch's first entry
    unsigned short* bin_of = reinterpret_cast<unsigned short*>(source + capacity);
    unsigned short* row_mark = reinterpret_cast<unsigned short*>(source);   // entry index -> row (relative), after a max-scan; read
                                                                            // for the last time before `source` is first written
    unsigned char* markers = reinterpret_cast<unsigned char*>(bin_of + capacity);
    __shared__ int s_plain;                     // this batch ranks its bins by comparison (the stable binning does not apply)

    const int tile = batch_tile[batch];
    const int row0 = batch_row[batch];
    // the next batch starts where this one ends — unless it belongs to the next tile
    const long long tile_end = min(static_cast<long long>(tile + 1) * sh.tile_rows, static_cast<long long>(sh.num_rows));
    const int row1 = batch + 1 < num_batches && batch_tile[batch + 1] == tile ? batch_row[batch + 1]
                                                                                : static_cast<int>(tile_end);
    const int tile_first = tile * sh.tile_rows;
    const long long entry0 = src.offset(row0), entry1 = src.offset(row1);
    // FAST: the batch's whole entry range fits the LDS arrays (always, unless long rows sit inside it): every
    // thread keeps its entries' columns and rows in registers between the phases, rows come from a scan
    const bool fast = entry1 - entry0 <= capacity;
    const int span = fast ? static_cast<int>(entry1 - entry0) : 0;
    // the fast path's column loads are issued first: they travel while the rows are being marked and scanned
    // Every wavefront takes a CONTIGUOUS share of the batch's entries, 64 at a time in source order (so that the stable
    // binning below can rely on "earlier wavefront, earlier instruction, lower lane = earlier entry").
    const int wave_id = threadIdx.x >> 6, lane_id = threadIdx.x & 63;
    const int per_wave = ((span + kBuildBlock / 64 - 1) / (kBuildBlock / 64) + 63) / 64 * 64;      // <= 64 * kBuildPerThread
    auto entry_of = [&](int u) {                       // index of this thread's u-th entry, or `span` (none)
        const int within = u * 64 + lane_id;
        return within < per_wave ? min(wave_id * per_wave + within, span) : span;
    };
    int my_col[kBuildPerThread];
#pragma unroll
    for (int u = 0; u < kBuildPerThread; ++u) {
        const int idx = entry_of(u);
        my_col[u] = idx < span ? src.col(entry0 + idx) : -1;
    }

    for (int i = threadIdx.x; i < S; i += kBuildBlock) {
        bin_cursor[i] = 0;
        bin_escapes[i] = 0;
        bin_ends[i] = 0;
    }
    for (int i = threadIdx.x; i < (kBuildBlock / 64) * S4; i += kBuildBlock) wave_count[i] = 0;
    if (threadIdx.x == 0) {
        s_overflow = 0;
        s_plain = fast && sh.stable_bins ? 0 : 1;
    }
    const bool rows_cached = Src::kSearchRows && !fast && row1 - row0 <= kBuildRowCache;
    if (rows_cached) {
        for (int r = row0 + threadIdx.x; r <= row1; r += kBuildBlock) s_row_cache[r - row0] = static_cast<int>(src.offset(r));
    }
    if (fast && Src::kSearchRows) {
        for (int i = threadIdx.x; i < span; i += kBuildBlock) row_mark[i] = 0;
    }
    __syncthreads();
    if (fast && Src::kSearchRows) {
        // every non-empty row marks its first entry; an inclusive max-scan then gives every entry its row
        for (int r = row0 + threadIdx.x; r < row1; r += kBuildBlock) {
            const long long b = src.offset(r);
            if (src.offset(r + 1) > b) row_mark[b - entry0] = static_cast<unsigned short>(r - row0);
        }
        __syncthreads();
        const int per = (span + kBuildBlock - 1) / kBuildBlock;
        const int lo = min(span, per * static_cast<int>(threadIdx.x)), hi = min(span, lo + per);
        int best = 0;
        for (int i = lo; i < hi; ++i) best = max(best, static_cast<int>(row_mark[i]));
        int unused;
        int run = block_exclusive_scan<true>(best, s_partial, &unused);
        for (int i = lo; i < hi; ++i) {
            run = max(run, static_cast<int>(row_mark[i]));
            row_mark[i] = static_cast<unsigned short>(run);
        }
        __syncthreads();
    }

    // SLOW path helpers (a batch whose entry range holds long rows): entries re-read per phase, rows searched
    auto row_of = [&](long long j) -> int {
        if (!Src::kSearchRows) return src.direct_row(j);
        int lo = row0, hi = row1;                  // offset(lo) <= j < offset(hi)
        if (rows_cached) {
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (s_row_cache[mid - row0] <= j) lo = mid; else hi = mid;
            }
        } else {
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                if (src.offset(mid) <= j) lo = mid; else hi = mid;
            }
        }
        return lo;
    };
    auto for_each_entry = [&](auto&& body) {
        for (long long j0 = entry0 + threadIdx.x; j0 < entry1; j0 += 4 * kBuildBlock) {
            int c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long j = j0 + static_cast<long long>(u) * kBuildBlock;
                c[u] = j < entry1 ? src.col(j) : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c[u] >= 0) body(j0 + static_cast<long long>(u) * kBuildBlock, c[u]);
            }
        }
    };
    // the row of entry j, or -1 when that row is long (then listed once, at its first entry, and its entries
    // are marked for the placing pass)
    auto short_row = [&](long long j, int row) -> int {
        if (!sh.any_long) return row;
        const long long begin = src.offset(row);
        if (src.offset(row + 1) - begin <= sh.long_row) return row;
        if (j == begin) long_rows[atomicAdd(num_long, 1)] = row;
        meta[j] = kMetaSkip;
        return -1;
    };

    // ---- histogram of the batch's short-row entries over the strips
    int my_lrow[kBuildPerThread];
    if (fast) {
#pragma unroll
        for (int u = 0; u < kBuildPerThread; ++u) {
            const int idx = entry_of(u);
            my_lrow[u] = 0;
            if (my_col[u] >= 0) {
                const long long j = entry0 + idx;
                const int row = short_row(j, Src::kSearchRows ? row0 + row_mark[idx] : src.direct_row(j));
                if (row < 0) {
                    my_col[u] = -1;
                } else {
                    my_lrow[u] = row - tile_first;
                    const int strip = my_col[u] >> sh.strip_shift;
                    atomicAdd(&bin_cursor[strip], 1);
                    // (bytes may run over into their neighbours when a bin holds more than 255: such a batch ranks by comparison)
                    atomicAdd(&wave_count[wave_id * S4 + (strip >> 2)], 1u << (8 * (strip & 3)));
                }
            }
        }
    } else {
        for_each_entry([&](long long j, int c) {
            if (sh.any_long && short_row(j, row_of(j)) < 0) return;
            atomicAdd(&bin_cursor[c >> sh.strip_shift], 1);
        });
    }
    __syncthreads();

    // ---- exclusive scan of the histogram: every thread owns a contiguous piece of the strips
    int total = 0;
    {
        const int per = (S + kBuildBlock - 1) / kBuildBlock;
        const int lo = min(S, per * static_cast<int>(threadIdx.x)), hi = min(S, lo + per);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += bin_cursor[i];
        int run = block_exclusive_scan<false>(sum, s_partial, &total);
        bool big = false;
        for (int i = lo; i < hi; ++i) {
            const int n = bin_cursor[i];
            bin_start[i] = run;
            bin_cursor[i] = run;
            run += n;
            big = big || n > 255;
        }
        if (big) s_plain = 1;           // a byte counter per wavefront and strip cannot hold this bin
        if (threadIdx.x == 0 && total > capacity) s_overflow = 1;
    }
    __syncthreads();
    if (s_overflow) return;          // cannot happen (the batch quota bounds the count); never write past LDS

    // STABLE BINNING (the usual case).  The entries of a batch arrive in (row, column) order — the order a bin must end up
    // in.  So instead of filling the bins in whatever order the atomics land and ranking every entry against its whole
    // bin afterwards (a loop as long as the longest bin of the wavefront: 2.4 of the kernel's 4.3 vector instructions per
    // entry, profiles/r03_build_counters.txt), every entry is sent straight to its final place: the count of its strip
    // in earlier wavefronts (the byte counters, turned into running offsets here) + its turn among its own wavefront's
    // entries (a returning LDS add; a wavefront issues its entries in source order).  The order in which ONE instruction's
    // lanes get their turn at the same counter is the hardware's; the bins are therefore checked afterwards (each slot
    // against its predecessor) and a batch that is out of order — also: rows whose columns are not ascending — falls back to
    // ranking by comparison.  Either way the layout is the same function of the matrix.
    const bool try_stable = s_plain == 0;
    if (try_stable) {
        // four strips at a time: the bytes of a word never carry into each other (every strip's total is <= 255 here)
        for (int i = threadIdx.x; i < S4; i += kBuildBlock) {
            unsigned int running = 0;
#pragma unroll
            for (int w = 0; w < kBuildBlock / 64; ++w) {
                const unsigned int mine = wave_count[w * S4 + i];
                wave_count[w * S4 + i] = running;
                running += mine;
            }
        }
        __syncthreads();
    }

    // ---- fill the bins (order inside a bin is arbitrary here; the ranking below fixes it)
    auto put = [&](int c, int lrow, unsigned int from) {
        const int strip = c >> sh.strip_shift;
        const int u = atomicAdd(&bin_cursor[strip], 1);
        keys[u] = (static_cast<unsigned int>(lrow) << 16) | static_cast<unsigned int>(c - (strip << sh.strip_shift));
        source[u] = from;
        bin_of[u] = static_cast<unsigned short>(strip);
    };
    if (try_stable) {
#pragma unroll
        for (int u = 0; u < kBuildPerThread; ++u) {
            if (my_col[u] >= 0) {
                const int strip = my_col[u] >> sh.strip_shift;
                const int shift = 8 * (strip & 3);
                const unsigned int before = atomicAdd(&wave_count[wave_id * S4 + (strip >> 2)], 1u << shift);
                const int slot = bin_start[strip] + static_cast<int>((before >> shift) & 0xFF);
                atomicAdd(&bin_cursor[strip], 1);          // (ends as the bin's end, like the unordered fill leaves it)
                keys[slot] = (static_cast<unsigned int>(my_lrow[u]) << 16) | static_cast<unsigned int>(my_col[u] - (strip << sh.strip_shift));
                source[slot] = static_cast<unsigned int>(entry_of(u));
                bin_of[slot] = static_cast<unsigned short>(strip);
            }
        }
    } else if (fast) {
#pragma unroll
        for (int u = 0; u < kBuildPerThread; ++u) {
            if (my_col[u] >= 0) put(my_col[u], my_lrow[u], entry_of(u));
        }
    } else {
        for_each_entry([&](long long j, int c) {
            const int row = row_of(j);
            if (sh.any_long && src.offset(row + 1) - src.offset(row) > sh.long_row) return;    // (listed above)
            put(c, row - tile_first, static_cast<unsigned int>(j - entry0));
        });
    }
    __syncthreads();

    // ---- rank inside the bin = number of slots ordered before this one; the largest key among them is the
    //      predecessor's.  Order: (row, column).  A row that stores one column twice (legal CSR) ties: such
    //      slots are ordered by their source index (the CSR order), found in a second, rare, loop.
    if (try_stable) {                     // is every slot behind its bin's previous one?  (row, column), twins by source index
        bool ordered = true;
#pragma unroll
        for (int k = 0; k < kBuildPerThread; ++k) {
            const int u = threadIdx.x + k * kBuildBlock;
            if (u < total && u > bin_start[bin_of[u]]) {
                const unsigned int pred = keys[u - 1], mine = keys[u];
                ordered = ordered && (pred < mine || (pred == mine && source[u - 1] < source[u]));
            }
        }
        if (!ordered) s_plain = 1;
        __syncthreads();
    }
    const bool stable = s_plain == 0;     // (the same for every thread: read after a barrier)
    int my_rank[kBuildPerThread], my_need[kBuildPerThread], my_delta[kBuildPerThread];
#pragma unroll
    for (int k = 0; k < kBuildPerThread; ++k) {
        const int u = threadIdx.x + k * kBuildBlock;
        my_rank[k] = -1;
        my_need[k] = 0;
        my_delta[k] = 0;
        if (u < total) {
            const int bin = bin_of[u];
            const int lo = bin_start[bin], hi = bin_cursor[bin];
            const unsigned int mine = keys[u];
            int rank = 0;
            unsigned int pred = 0;
            if (stable) {                 // the slot IS the rank
                rank = u - lo;
                pred = rank > 0 ? keys[u - 1] : 0u;
            } else {
                int ties = 0;
                for (int v = lo; v < hi; ++v) {
                    const unsigned int key = keys[v];
                    const bool less = key < mine;
                    rank += less;
                    pred = less ? max(pred, key) : pred;
                    ties += key == mine;
                }
                if (ties > 1) {           // duplicate (row, column): order the twins by source index
                    const unsigned int me = source[u];
                    for (int v = lo; v < hi; ++v) {
                        if (keys[v] == mine && source[v] < me) {
                            ++rank;
                            pred = mine;
                        }
                    }
                }
            }
            const int lrow = static_cast<int>(mine >> 16);
            my_rank[k] = rank;
            if (rank > 0) {
                const int gap = lrow - static_cast<int>(pred >> 16);
                my_need[k] = gap / kSkip;                 // skip markers in front of this slot
                my_delta[k] = gap - my_need[k] * kSkip;
                if (my_need[k]) atomicAdd(&bin_escapes[bin], my_need[k]);
            } else {
                atomicOr(&bin_ends[bin], lrow << 16);     // exactly one slot per bin comes first ...
            }
            if (rank == hi - lo - 1) atomicOr(&bin_ends[bin], lrow);     // ... and exactly one last
            markers[u] = static_cast<unsigned char>(my_need[k]);
        }
    }
    __syncthreads();

    // ---- the per-entry records for the placing pass
#pragma unroll
    for (int k = 0; k < kBuildPerThread; ++k) {
        const int u = threadIdx.x + k * kBuildBlock;
        if (u < total) {
            const int bin = bin_of[u];
            const unsigned int mine = keys[u];
            unsigned int record;
            if (my_rank[k] == 0) {
                record = kMetaFirst | (mine >> 16);
            } else {
                int in_front = my_rank[k] + my_need[k];
                if (bin_escapes[bin] != my_need[k]) {       // rare: other slots of this bin need markers too
                    const unsigned int me = source[u];
                    for (int v = bin_start[bin]; v < bin_cursor[bin]; ++v) {
                        const unsigned int key = keys[v];
                        if (key < mine || (key == mine && source[v] < me)) in_front += markers[v];
                    }
                }
                record = (static_cast<unsigned int>(in_front) << 16) | (static_cast<unsigned int>(my_need[k]) << 8) |
                         static_cast<unsigned int>(my_delta[k]);
            }
            meta[entry0 + source[u]] = record;
        }
    }
    for (int i = threadIdx.x; i < S; i += kBuildBlock) {
        GroupCount g;
        g.count = static_cast<unsigned short>(bin_cursor[i] - bin_start[i]);
        g.first = static_cast<unsigned short>(static_cast<unsigned int>(bin_ends[i]) >> 16);
        g.last = static_cast<unsigned short>(bin_ends[i] & 0xFFFF);
        g.escapes = static_cast<unsigned short>(bin_escapes[i]);
        uint2 packed;
        __builtin_memcpy(&packed, &g, sizeof(g));
        groups[static_cast<long long>(batch) * S + i] = packed;
    }
}

// The placing pass: no sorting any more — every entry of the batch goes to cell begin + group offset + the
// position the ranking pass recorded, preceded by its skip markers.  Dynamic LDS: 12 bytes per strip (the
// batch's group records and its tile's cell begins).
template <typename Src>
__global__ __launch_bounds__(kBuildBlock)
void batch_place_kernel(Src src, BuildShape sh, int num_batches,
                        const int* __restrict__ batch_row, const int* __restrict__ batch_tile,
                        const uint2* __restrict__ groups,              // [batches * strips] GroupPlace
                        const unsigned int* __restrict__ meta, const int2* __restrict__ cells_t,
                        float* __restrict__ a_val, unsigned short* __restrict__ a_lcol,
                        unsigned char* __restrict__ a_drow,
                        const int* __restrict__ todo /*null: every batch; else [0] = how many, [1 ...] = which (left by the staged pass)*/) {
    extern __shared__ int place_lds[];
    const int S = sh.num_strips;
    uint2* place = reinterpret_cast<uint2*>(place_lds);
    int* cell_begin = place_lds + 2 * S;
    // behind the staged pass only the batches it listed are left (usually none): a fixed grid walks the list — a workgroup
    // per batch just to find out that there is nothing to do cost ~40 us of launches on C5
    const int work = todo ? todo[0] : xcd_grid(num_batches);
    for (int position = blockIdx.x; position < work; position += gridDim.x) {
    const int batch = todo ? todo[1 + position] : xcd_contiguous(position, num_batches);
    if (batch < 0) continue;
    __syncthreads();                           // the previous batch's LDS records are no longer read
    const int tile = batch_tile[batch];
    const int row0 = batch_row[batch];
    const long long tile_end = min(static_cast<long long>(tile + 1) * sh.tile_rows, static_cast<long long>(sh.num_rows));
    const int row1 = batch + 1 < num_batches && batch_tile[batch + 1] == tile ? batch_row[batch + 1]
                                                                                : static_cast<int>(tile_end);
    const long long entry0 = src.offset(row0), entry1 = src.offset(row1);
    for (int i = threadIdx.x; i < S; i += kBuildBlock) {
        place[i] = groups[static_cast<long long>(batch) * S + i];
        cell_begin[i] = cells_t[static_cast<long long>(tile) * S + i].x;     // (tile-major table: one contiguous read; the strip-major
                                                                          //  offsets sit num_tiles ints apart: a line per strip)
    }
    __syncthreads();
    for (long long j0 = entry0 + threadIdx.x; j0 < entry1; j0 += 4 * kBuildBlock) {
        int c[4];
        unsigned int m[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long j = j0 + static_cast<long long>(u) * kBuildBlock;
            c[u] = -1;
            if (j < entry1) {
                c[u] = src.col(j);
                m[u] = meta[j];
                v[u] = a_val ? src.val(j) : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c[u] < 0 || m[u] == kMetaSkip) continue;
            const int strip = c[u] >> sh.strip_shift;
            GroupPlace p;
            __builtin_memcpy(&p, &place[strip], sizeof(p));
            long long at = static_cast<long long>(cell_begin[strip]) + p.rel;
            int need, delta;
            if (m[u] & kMetaFirst) {
                need = p.lead;
                delta = static_cast<int>(m[u] & 0xFFFF) - p.prev_last - need * kSkip;
            } else {
                need = (m[u] >> 8) & 0xFF;
                delta = m[u] & 0xFF;
                at += p.lead + (m[u] >> 16) - need;
            }
            for (int k = 0; k < need; ++k) {
                if (a_val) a_val[at + k] = 0.0f;
                a_lcol[at + k] = 0;
                a_drow[at + k] = kSkip;
            }
            if (a_val) a_val[at + need] = v[u];
            a_lcol[at + need] = static_cast<unsigned short>(c[u] - (strip << sh.strip_shift));
            a_drow[at + need] = static_cast<unsigned char>(delta);
        }
    }
    }
}

// The same placing pass with the batch's slots assembled in LDS first, in destination order, so that the global
// stores leave the workgroup as contiguous segments (one per group and array) instead of one element per lane:
// the scattered form above issues ~3 partial-line writes per entry (C5: 480 M of them, 3.8 ms), this one ~3 per
// GROUP.  Takes the batches whose entries a workgroup can hold in registers (entry range <= capacity) and whose
// slots (markers included) fit the staging area; every other batch is left to batch_place_kernel (`todo` flag).
// Dynamic LDS: per strip place (8 B), cell begin, slot count, local offset (4 B each); per staged slot value f32,
// local column u16, strip u16, row delta u8.
constexpr int kStageBytesPerStrip = 20, kStageBytesPerSlot = 9;
template <typename Src>
__global__ __launch_bounds__(kBuildBlock, 8)
void batch_place_staged_kernel(Src src, BuildShape sh, int num_batches, int capacity, int stage_slots,
                               const int* __restrict__ batch_row, const int* __restrict__ batch_tile,
                               const uint2* __restrict__ groups,              // [batches * strips] GroupPlace
                               const unsigned int* __restrict__ meta, const int2* __restrict__ cells_t,
                               float* __restrict__ a_val, unsigned short* __restrict__ a_lcol,
                               unsigned char* __restrict__ a_drow, int* __restrict__ todo /*[0] count, [1 ...] batches left over*/) {
    extern __shared__ int stage_lds[];
    __shared__ int s_partial[kBuildBlock / 64];
    const int batch = xcd_contiguous(blockIdx.x, num_batches);
    if (batch < 0) return;
    const int S = sh.num_strips;
    uint2* place = reinterpret_cast<uint2*>(stage_lds);                 // [S]
    int* cell_begin = stage_lds + 2 * S;                                 // [S]
    int* count = stage_lds + 3 * S;                                      // [S] slots of the batch per strip
    int* local = stage_lds + 4 * S;                                      // [S] first staged slot of the strip
    float* st_val = reinterpret_cast<float*>(stage_lds + 5 * S);         // [stage_slots]
    unsigned short* st_lcol = reinterpret_cast<unsigned short*>(st_val + stage_slots);
    unsigned short* st_strip = st_lcol + stage_slots;
    unsigned char* st_drow = reinterpret_cast<unsigned char*>(st_strip + stage_slots);

    const int tile = batch_tile[batch];
    const int row0 = batch_row[batch];
    const long long tile_end = min(static_cast<long long>(tile + 1) * sh.tile_rows, static_cast<long long>(sh.num_rows));
    const int row1 = batch + 1 < num_batches && batch_tile[batch + 1] == tile ? batch_row[batch + 1]
                                                                                : static_cast<int>(tile_end);
    const long long entry0 = src.offset(row0), entry1 = src.offset(row1);
    if (entry1 - entry0 > capacity) {          // (a batch with long rows inside: the scattered kernel takes it)
        if (threadIdx.x == 0) todo[1 + atomicAdd(&todo[0], 1)] = batch;
        return;
    }
    const int span = static_cast<int>(entry1 - entry0);
    for (int i = threadIdx.x; i < S; i += kBuildBlock) {
        place[i] = groups[static_cast<long long>(batch) * S + i];
        cell_begin[i] = cells_t[static_cast<long long>(tile) * S + i].x;     // (tile-major table: one contiguous read; the strip-major
                                                                          //  offsets sit num_tiles ints apart: a line per strip)
        count[i] = 0;
    }
    __syncthreads();

    // every thread keeps its entries: strip, local column, slots it needs (itself + the markers in front of it),
    // position inside its group
    int my_strip[kBuildPerThread], my_front[kBuildPerThread], my_need[kBuildPerThread], my_delta[kBuildPerThread];
    float my_val[kBuildPerThread];
    unsigned short my_lcol[kBuildPerThread];
#pragma unroll
    for (int u = 0; u < kBuildPerThread; ++u) {
        const int idx = threadIdx.x + u * kBuildBlock;
        my_strip[u] = -1;
        if (idx < span) {
            const long long j = entry0 + idx;
            const int c = src.col(j);
            const unsigned int m = meta[j];
            if (c >= 0 && m != kMetaSkip) {
                const int strip = c >> sh.strip_shift;
                GroupPlace p;
                __builtin_memcpy(&p, &place[strip], sizeof(p));
                my_strip[u] = strip;
                my_lcol[u] = static_cast<unsigned short>(c - (strip << sh.strip_shift));
                my_val[u] = a_val ? src.val(j) : 0.0f;
                if (m & kMetaFirst) {
                    my_need[u] = p.lead;
                    my_delta[u] = static_cast<int>(m & 0xFFFF) - p.prev_last - my_need[u] * kSkip;
                    my_front[u] = 0;
                } else {
                    my_need[u] = (m >> 8) & 0xFF;
                    my_delta[u] = m & 0xFF;
                    my_front[u] = p.lead + static_cast<int>(m >> 16) - my_need[u];
                }
                atomicAdd(&count[strip], 1 + my_need[u]);
            }
        }
    }
    __syncthreads();

    // exclusive scan of the per-strip slot counts (every thread owns a contiguous piece of the strips)
    int total;
    {
        const int per = (S + kBuildBlock - 1) / kBuildBlock;
        const int lo = min(S, per * static_cast<int>(threadIdx.x)), hi = min(S, lo + per);
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += count[i];
        int run = block_exclusive_scan<false>(sum, s_partial, &total);
        for (int i = lo; i < hi; ++i) {
            local[i] = run;
            run += count[i];
        }
    }
    __syncthreads();
    if (total > stage_slots) {                 // (markers galore: more slots than the staging area holds)
        if (threadIdx.x == 0) todo[1 + atomicAdd(&todo[0], 1)] = batch;
        return;
    }

    // assemble the batch's slots in destination order
#pragma unroll
    for (int u = 0; u < kBuildPerThread; ++u) {
        if (my_strip[u] < 0) continue;
        const int at = local[my_strip[u]] + my_front[u];
        for (int k = 0; k < my_need[u]; ++k) {
            st_val[at + k] = 0.0f;
            st_lcol[at + k] = 0;
            st_strip[at + k] = static_cast<unsigned short>(my_strip[u]);
            st_drow[at + k] = kSkip;
        }
        st_val[at + my_need[u]] = my_val[u];
        st_lcol[at + my_need[u]] = my_lcol[u];
        st_strip[at + my_need[u]] = static_cast<unsigned short>(my_strip[u]);
        st_drow[at + my_need[u]] = static_cast<unsigned char>(my_delta[u]);
    }
    __syncthreads();

    // ... and write them out: consecutive lanes, consecutive slots of a group, consecutive addresses
    for (int u = threadIdx.x; u < total; u += kBuildBlock) {
        const int strip = st_strip[u];
        GroupPlace p;
        __builtin_memcpy(&p, &place[strip], sizeof(p));
        const long long at = static_cast<long long>(cell_begin[strip]) + p.rel + (u - local[strip]);
        if (a_val) a_val[at] = st_val[u];
        a_lcol[at] = st_lcol[u];
        a_drow[at] = st_drow[u];
    }
}

// One thread per cell (tile, strip): walks the tile's batches in row order, places every group inside the
// cell (markers between groups included) and records the cell's slot count.
__global__ __launch_bounds__(kBlock)
void cell_place_kernel(int num_tiles, int num_strips, const int* __restrict__ tile_batch,
                       uint2* __restrict__ groups, int* __restrict__ cell_slots /*strip-major*/,
                       unsigned long long* __restrict__ entry_total) {
    const long long id = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
    unsigned long long mine = 0;
    if (id < static_cast<long long>(num_tiles) * num_strips) {
        const int tile = static_cast<int>(id / num_strips), strip = static_cast<int>(id % num_strips);
        int last = 0;
        unsigned int total = 0;
        const int b_end = tile_batch[tile + 1];
        uint2 ahead = make_uint2(0, 0);       // the next batch's record is fetched before this one's is rewritten (other addresses)
        if (tile_batch[tile] < b_end) ahead = groups[static_cast<long long>(tile_batch[tile]) * num_strips + strip];
        for (int b = tile_batch[tile]; b < b_end; ++b) {
            uint2* slot = groups + static_cast<long long>(b) * num_strips + strip;
            const uint2 raw = ahead;
            if (b + 1 < b_end) ahead = groups[static_cast<long long>(b + 1) * num_strips + strip];
            GroupCount g;
            __builtin_memcpy(&g, &raw, sizeof(g));
            GroupPlace p;
            p.rel = total;
            p.prev_last = static_cast<unsigned short>(last);
            p.lead = 0;
            if (g.count) {
                p.lead = static_cast<unsigned short>((g.first - last) / kSkip);
                total += g.count + g.escapes + p.lead;
                last = g.last;
                mine += g.count;
            }
            uint2 packed;
            __builtin_memcpy(&packed, &p, sizeof(p));
            *slot = packed;
        }
        cell_slots[static_cast<long long>(strip) * num_tiles + tile] = static_cast<int>(total);
    }
    // one atomic per workgroup (ten thousand wavefronts adding to one address serialise at the memory side)
    __shared__ unsigned long long s_mine[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63) == 0) s_mine[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < kBlock / 64; ++w) all += s_mine[w];
        if (all) atomicAdd(entry_total, all);
    }
}

// exclusive scan of round_up_4(in[i]) in three launches: block sums, scan of the sums, block scans
constexpr int kScanBlock = 1024, kScanPerThread = 4, kScanTile = kScanBlock * kScanPerThread;
__device__ __forceinline__ int padded4(int v) { return (v + 3) & ~3; }

__global__ __launch_bounds__(kScanBlock)
void scan_sums_kernel(const int* __restrict__ in, long long n, long long* __restrict__ block_sum) {
    __shared__ long long s_wave[kScanBlock / 64];
    const long long first = static_cast<long long>(blockIdx.x) * kScanTile + threadIdx.x * kScanPerThread;
    long long sum = 0;
    for (int k = 0; k < kScanPerThread; ++k) if (first + k < n) sum += padded4(in[first + k]);
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long total = 0;
        for (int w = 0; w < kScanBlock / 64; ++w) total += s_wave[w];
        block_sum[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kScanBlock)
void scan_top_kernel(long long* __restrict__ block_sum, int blocks, long long* __restrict__ grand_total) {
    __shared__ long long s_part[kScanBlock];
    const int per = (blocks + kScanBlock - 1) / kScanBlock;
    const int lo = min(blocks, per * static_cast<int>(threadIdx.x)), hi = min(blocks, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += block_sum[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        const long long add = static_cast<int>(threadIdx.x) >= off ? s_part[threadIdx.x - off] : 0;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (int i = lo; i < hi; ++i) {
        const long long v = block_sum[i];
        block_sum[i] = run;
        run += v;
    }
    if (threadIdx.x == kScanBlock - 1) *grand_total = s_part[kScanBlock - 1];
}

__global__ __launch_bounds__(kScanBlock)
void scan_apply_kernel(const int* __restrict__ in, long long n, const long long* __restrict__ block_sum,
                       int* __restrict__ out /*[n + 1]*/) {
    __shared__ int s_part[kScanBlock];
    const long long first = static_cast<long long>(blockIdx.x) * kScanTile + threadIdx.x * kScanPerThread;
    int v[kScanPerThread], sum = 0;
    for (int k = 0; k < kScanPerThread; ++k) {
        v[k] = first + k < n ? padded4(in[first + k]) : 0;
        sum += v[k];
    }
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        const int add = static_cast<int>(threadIdx.x) >= off ? s_part[threadIdx.x - off] : 0;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = block_sum[blockIdx.x] + (threadIdx.x ? s_part[threadIdx.x - 1] : 0);
    for (int k = 0; k < kScanPerThread; ++k) {
        if (first + k < n) out[first + k] = static_cast<int>(run);
        run += v[k];
        if (first + k == n - 1) out[n] = static_cast<int>(run);
    }
}

// counts[0 .. n) -> exclusive prefix sums in place, counts[n] = total.  One workgroup, each thread a contiguous piece.
__global__ __launch_bounds__(kScanBlock)
void exclusive_scan_small_kernel(int* __restrict__ counts, int n) {
    __shared__ long long s_part[kScanBlock];
    const int per = (n + kScanBlock - 1) / kScanBlock;
    const int lo = min(n, per * static_cast<int>(threadIdx.x)), hi = min(n, lo + per);
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += counts[i];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kScanBlock; off <<= 1) {
        const long long add = static_cast<int>(threadIdx.x) >= off ? s_part[threadIdx.x - off] : 0;
        __syncthreads();
        s_part[threadIdx.x] += add;
        __syncthreads();
    }
    long long run = threadIdx.x ? s_part[threadIdx.x - 1] : 0;
    for (int i = lo; i < hi; ++i) {
        const int v = counts[i];
        counts[i] = static_cast<int>(run);
        run += v;
    }
    if (threadIdx.x == kScanBlock - 1) counts[n] = static_cast<int>(s_part[kScanBlock - 1]);
}

// the padding slots at the end of every cell (and nothing else): skip markers
__global__ __launch_bounds__(kBlock)
void cell_padding_kernel(const int* __restrict__ cell_slots, const int* __restrict__ offs, long long cells,
                         float* __restrict__ a_val, unsigned short* __restrict__ a_lcol,
                         unsigned char* __restrict__ a_drow) {
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < cells;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int used = cell_slots[i];
        for (int k = used; k < padded4(used); ++k) {
            const long long at = static_cast<long long>(offs[i]) + k;
            if (a_val) a_val[at] = 0.0f;
            a_lcol[at] = 0;
            a_drow[at] = kSkip;
        }
    }
}

// cells_t[tile * num_strips + strip] = (begin, length) of the cell's run;
// strip_begin[s] = first entry of strip s (s <= num_strips)
__global__ __launch_bounds__(kBlock)
void cell_table_kernel(const int* __restrict__ offs, int num_strips, int num_tiles,
                       int2* __restrict__ cells_t, int* __restrict__ strip_begin) {
    const long long cells = static_cast<long long>(num_strips) * num_tiles;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i <= cells;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        if (i < cells) {
            const long long tile = i / num_strips, strip = i % num_strips;
            const long long cell = strip * num_tiles + tile;
            cells_t[i] = make_int2(offs[cell], offs[cell + 1] - offs[cell]);
        }
        if (i <= num_strips) strip_begin[i] = offs[i * num_tiles];
    }
}

// Lays out the passes of every (tile, wavefront): FILL = false counts them (-> pass_count[tile * 16 + wave]), FILL = true
// writes their descriptors at pass_first[tile * 16 + wave] and, beside each, the pass's 64 row-delta words in lane order
// (pass_word, tiled_layout.h).  One 1024-thread workgroup per tile, wavefront w does the share
// of wavefront w of the phase-2 workgroup.  The (begin, length) records of a wavefront's runs come 64 at a time (lane l holds
// run window_first + l, read back with v_readlane); a pass never straddles two such windows.
template <bool FILL>
__global__ __launch_bounds__(kReduceThreads)
void pass_layout_kernel(int num_tiles, int num_strips, const int2* __restrict__ cells_t,
                        const unsigned char* __restrict__ a_drow,
                        int* __restrict__ pass_count, const int* __restrict__ pass_first, PassDesc* __restrict__ desc,
                        unsigned int* __restrict__ pass_word) {
    const int tile_index = blockIdx.x;
    if (tile_index >= num_tiles) return;
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    int run_lo, run_hi;
    wave_runs(num_strips, wave, &run_lo, &run_hi);
    const int2* mine = cells_t + static_cast<long long>(tile_index) * num_strips;
    int passes = 0;
    long long out = FILL ? pass_first[tile_index * kReduceWaves + wave] : 0;
    for (int window_first = run_lo; window_first < run_hi; window_first += 64) {
        const int2 window = window_first + lane < run_hi ? mine[window_first + lane] : make_int2(0, 0);
        const int window_runs = min(64, run_hi - window_first);
        int next_run = 0, cur_begin = 0, cur_len = 0, off = 0;     // the stream cursor (wave-uniform)
        int row_carry = 0;                                         // the row the open run has reached
        for (;;) {
            int base[kPassSegs], start[kPassSegs];
            int filled = 0, last = 0;
            bool fresh0 = true;
#pragma unroll
            for (int k = 0; k < kPassSegs; ++k) {
                while (off >= cur_len && next_run < window_runs) {       // the next run that holds slots (banded matrices: most are empty)
                    cur_begin = __builtin_amdgcn_readlane(window.x, next_run);
                    cur_len = __builtin_amdgcn_readlane(window.y, next_run);
                    off = 0;
                    ++next_run;
                }
                const int take = max(min(cur_len - off, kPassSlots - filled), 0);
                if (k == 0) fresh0 = off == 0;
                base[k] = cur_begin + off - filled;
                start[k] = filled >> 2;
                last = take > 0 ? k : last;
                filled += take;
                off += take;
            }
            if (filled == 0) break;
            ++passes;
            if (!FILL) continue;
            const bool open_end = off < cur_len;
            const int groups = filled >> 2;
            // the delta bytes of the pass: what phase 2 will read, lane by lane
            const int at = min(lane, groups - 1);
            int mine_base = base[0];
#pragma unroll
            for (int k = 1; k < kPassSegs; ++k) mine_base = at >= start[k] ? base[k] : mine_base;
            const unsigned int word = lane < groups ? *reinterpret_cast<const unsigned int*>(a_drow + mine_base + 4 * at) : 0u;
            pass_word[out * 64 + lane] = lane < groups ? word : 0xFFFFFFFFu;     // past the end: four skip markers
            const int sum = static_cast<int>((word & 0xFF) + ((word >> 8) & 0xFF) + ((word >> 16) & 0xFF) + (word >> 24));
            const int incl = wave_inclusive_scan(sum);
            // row in front of each segment, and the delta sums in front of it
            int adj[kPassSegs];
            int origin = fresh0 ? 0 : row_carry;
            adj[0] = origin;
#pragma unroll
            for (int k = 1; k < kPassSegs; ++k) {
                const int before = start[k] > 0 ? __builtin_amdgcn_readlane(incl, max(start[k] - 1, 0)) : 0;
                adj[k] = -before;                          // a segment behind the first starts a run: its rows count from 0
                origin = k <= last ? adj[k] : origin;
            }
            row_carry = open_end ? origin + __builtin_amdgcn_readlane(incl, groups - 1) : 0;
            if (lane == 0) {
                PassDesc d;
#pragma unroll
                for (int k = 0; k < kPassSegs; ++k) {
                    d.base[k] = base[k];
                    d.adj[k] = adj[k];
                }
                d.geom = static_cast<unsigned int>(start[1]) | static_cast<unsigned int>(start[2]) << 8 | static_cast<unsigned int>(groups) << 16;
                d.reserved = 0;
                desc[out] = d;
            }
            ++out;
        }
    }
    if (!FILL && lane == 0) pass_count[tile_index * kReduceWaves + wave] = passes;
}

// The build's temporaries are carved out of two allocations: every hipFree synchronises the device, and eleven
// of them were ~0.8 ms of a 5.5 ms build.
struct BuildArena {
    DevBuf<char> base;
    size_t size = 0, used = 0;
    hipError_t reserve() { return dev_alloc(&base, static_cast<long long>(size)); }
    static size_t padded(size_t bytes) { return (bytes + 255) / 256 * 256; }
    template <typename T>
    T* take(long long count) {
        T* p = reinterpret_cast<T*>(base.get() + used);
        used += padded(static_cast<size_t>(std::max<long long>(count, 1)) * sizeof(T));
        return p;
    }
};

// the device passes of the build for one entry source
template <typename Src>
hipError_t build_cells_from(const Src& dev_src, bool has_long_path, TiledPlan* plan, BuiltCells* out, hipStream_t s) {
    BuildTrace trace;
    const int S = plan->num_strips, T = plan->num_tiles;
    const long long cells = static_cast<long long>(S) * T;

    int *d_small = nullptr;            // [0] longest row, [1] long-row count
    int *tile_batch = nullptr, *batch_row = nullptr, *batch_tile = nullptr, *cell_slots = nullptr, *offs = nullptr;
    int *strip_begin = nullptr;
    long long* block_sum = nullptr;    // scan scratch; [blocks] sums, then [blocks] grand total, [blocks + 1] entry count
    uint2* groups = nullptr;
    unsigned int* meta = nullptr;      // per-entry records between the ranking and the placing pass
    int* place_todo = nullptr;             // [0] how many, [1 ...] which batches the staged placing pass left to the scattered one
    BuildArena first, second;     // what is known up front; what depends on the batch count
    const int scan_blocks = static_cast<int>((cells + kScanTile - 1) / kScanTile);
    const int tile_scan_blocks = (T + kScanTile - 1) / kScanTile;

    const long long scan_slots = std::max(scan_blocks, tile_scan_blocks) + 2;
    first.size = BuildArena::padded(2 * sizeof(int)) + BuildArena::padded((static_cast<size_t>(T) + 1) * sizeof(int)) +
                 BuildArena::padded(static_cast<size_t>(cells) * sizeof(int)) + BuildArena::padded((static_cast<size_t>(cells) + 1) * sizeof(int)) +
                 BuildArena::padded(static_cast<size_t>(scan_slots) * sizeof(long long));
    hipError_t e = first.reserve();
    if (e == hipSuccess) {
        d_small = first.take<int>(2);
        tile_batch = first.take<int>(static_cast<long long>(T) + 1);
        cell_slots = first.take<int>(cells);
        offs = first.take<int>(cells + 1);
        block_sum = first.take<long long>(scan_slots);
        e = dev_alloc(&out->strip_begin, S + 1);     // (outlives this function: the fold probe reads it)
        strip_begin = out->strip_begin.get();
    }
    if (e == hipSuccess) e = hipMemsetAsync(d_small, 0, 2 * sizeof(int), s);
    if (e != hipSuccess) return e;

    // ---- batch geometry: how many entries a builder workgroup can hold in LDS
    const int lds_bytes = S <= 1024 ? kBuildLdsSmall : kBuildLdsLarge;
    int capacity = (lds_bytes - kBuildBinWords * 4 * S - kBuildWaveCountBytes * ((S + 3) / 4 * 4)) / kBuildEntryBytes / 64 * 64;
    if (capacity < 512) return hipErrorInvalidValue;
    capacity = std::min(capacity, kBuildMaxCapacity);        // what a workgroup's threads keep in registers
    max_row_kernel<<<std::min(1024, (plan->num_rows + kBlock - 1) / kBlock), kBlock, 0, s>>>(dev_src, plan->num_rows, d_small);
    int longest = 0;
    e = hipMemcpyAsync(&longest, d_small, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    trace.mark("allocations + longest row");
    const int longest_short = std::min(longest, plan->long_row);
    if (longest_short >= capacity) plan->long_row = capacity / 2;      // (rows that long go the direct way)
    BuildShape sh;
    sh.num_rows = plan->num_rows;
    sh.num_tiles = T;
    sh.num_strips = S;
    sh.strip_shift = __builtin_ctz(static_cast<unsigned>(plan->strip_cols));
    sh.tile_rows = plan->tile_rows;
    sh.long_row = plan->long_row;
    sh.quota = std::max(64, capacity - std::min(longest, plan->long_row));
    sh.any_long = longest > plan->long_row ? 1 : 0;
    sh.stable_bins = 1;
    if (debug_is("rank", "plain")) sh.stable_bins = 0;

    tile_batches_kernel<<<(T + kBlock - 1) / kBlock, kBlock, 0, s>>>(dev_src, sh, tile_batch);
    // exclusive scan of the per-tile batch counts (one workgroup: T is at most a few hundred thousand)
    exclusive_scan_small_kernel<<<1, kScanBlock, 0, s>>>(tile_batch, T);
    int num_batches = 0;
    e = hipMemcpyAsync(&num_batches, tile_batch + T, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;

    trace.mark("batch counts");
    const long long group_count = static_cast<long long>(num_batches) * S;
    second.size = BuildArena::padded((static_cast<size_t>(num_batches) + 1) * sizeof(int)) +
                  BuildArena::padded(static_cast<size_t>(std::max(num_batches, 1)) * sizeof(int)) +
                  BuildArena::padded(static_cast<size_t>(std::max<long long>(group_count, 1)) * sizeof(uint2)) +
                  BuildArena::padded(static_cast<size_t>(std::max<long long>(plan->csr_nnz, 1)) * sizeof(unsigned int)) +
                  BuildArena::padded((static_cast<size_t>(std::max(num_batches, 1)) + 1) * sizeof(int));
    e = second.reserve();
    if (e == hipSuccess) {
        batch_row = second.take<int>(static_cast<long long>(num_batches) + 1);
        batch_tile = second.take<int>(num_batches);
        groups = second.take<uint2>(group_count);
        meta = second.take<unsigned int>(plan->csr_nnz);
        place_todo = second.take<int>(static_cast<long long>(num_batches) + 1);
    }
    if (e == hipSuccess && has_long_path) {
        e = dev_alloc(&plan->long_rows, plan->csr_nnz / std::max(plan->long_row, 1) + 1);
    }
    if (e != hipSuccess) return e;
    batch_rows_kernel<<<T, kBlock, 0, s>>>(dev_src, sh, tile_batch, batch_row, batch_tile);

    trace.mark("allocations (batches)");
    // ---- ranking pass: group sizes + per-entry records; cell placement; scan
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&batch_rank_kernel<Src>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    batch_rank_kernel<Src><<<xcd_grid(num_batches), kBuildBlock, lds_bytes, s>>>(
        dev_src, sh, num_batches, capacity, batch_row, batch_tile, groups, meta, plan->long_rows.get(), d_small + 1);
    unsigned long long* entry_total = reinterpret_cast<unsigned long long*>(block_sum + scan_blocks + 1);
    e = hipMemsetAsync(entry_total, 0, sizeof(unsigned long long), s);
    cell_place_kernel<<<static_cast<int>((cells + kBlock - 1) / kBlock), kBlock, 0, s>>>(T, S, tile_batch, groups, cell_slots,
                                                                                       entry_total);
    scan_sums_kernel<<<scan_blocks, kScanBlock, 0, s>>>(cell_slots, cells, block_sum);
    scan_top_kernel<<<1, kScanBlock, 0, s>>>(block_sum, scan_blocks, block_sum + scan_blocks);
    scan_apply_kernel<<<scan_blocks, kScanBlock, 0, s>>>(cell_slots, cells, block_sum, offs);
    if (e == hipSuccess) e = hipGetLastError();
    long long totals[2] = {0, 0};          // slots, entries
    int num_long = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(totals, block_sum + scan_blocks, 2 * sizeof(long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&num_long, d_small + 1, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    trace.mark("ranking + scans (sync)");
    if (totals[0] >= 0x7fffffffLL - 64) return hipErrorInvalidValue;       // slot indices are 32-bit
    plan->nnz = totals[0];
    plan->entries = totals[1];
    plan->num_long = num_long;

    // ---- placing pass: write the slots
    e = dev_alloc(&plan->a_val, plan->nnz + 8);
    // + 8: the 16-byte loads of a run's last group stay inside the allocation whatever its alignment
    if (e == hipSuccess) e = dev_alloc(&plan->a_lcol, plan->nnz + 8);
    if (e == hipSuccess) e = dev_alloc(&plan->a_drow, plan->nnz + 8);
    if (e == hipSuccess) e = dev_alloc(&plan->cells_t, 2 * cells);
    const int pass_waves = T * kReduceWaves;
    if (e == hipSuccess) e = dev_alloc(&plan->pass_first, static_cast<long long>(pass_waves) + 1);
    if (e != hipSuccess) return e;
    float* a_val = plan->a_val.get();
    unsigned short* a_lcol = plan->a_lcol.get();
    unsigned char* a_drow = plan->a_drow.get();
    int2* cells_t = reinterpret_cast<int2*>(plan->cells_t.get());
    int* pass_first = plan->pass_first.get();
    {   // the tile-major cell table first: the placing kernels read their tile's cell begins from it (one contiguous read)
        const int grid = static_cast<int>(std::min<long long>((cells + kBlock) / kBlock, 4096));
        cell_table_kernel<<<grid, kBlock, 0, s>>>(offs, S, T, cells_t, strip_begin);
        // phase 2's passes are a function of the cell table alone: counted and scanned here, beside the placing pass, so that
        // their total arrives with this function's last synchronisation (the descriptors are written by build_plan)
        pass_layout_kernel<false><<<T, kReduceThreads, 0, s>>>(T, S, cells_t, nullptr, pass_first, nullptr, nullptr, nullptr);
        exclusive_scan_small_kernel<<<1, kScanBlock, 0, s>>>(pass_first, pass_waves);
    }
    if (plan->nnz > 0) {
        // staged placing pass (contiguous segments); the batches it cannot hold are flagged for the scattered one
        bool staged = true;
        if (debug_is("place", "scattered")) staged = false;
        int* todo = place_todo;
        if (staged) {
            const int stage_slots = (capacity + 1024 + 63) / 64 * 64;
            const size_t stage_lds = static_cast<size_t>(kStageBytesPerStrip) * S + static_cast<size_t>(kStageBytesPerSlot) * stage_slots;
            staged = stage_lds + sizeof(int) * kBuildBlock + 64 <= 160 * 1024;
            if (staged) e = hipMemsetAsync(todo, 0, sizeof(int), s);
            if (staged && e == hipSuccess) {
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(&batch_place_staged_kernel<Src>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(stage_lds));
            }
            if (e != hipSuccess) return e;
            if (staged) {
                batch_place_staged_kernel<Src><<<xcd_grid(num_batches), kBuildBlock, stage_lds, s>>>(
                    dev_src, sh, num_batches, capacity, stage_slots, batch_row, batch_tile, groups, meta, cells_t, a_val, a_lcol, a_drow, todo);
            }
        }
        batch_place_kernel<Src><<<staged ? std::min(xcd_grid(num_batches), 512) : xcd_grid(num_batches), kBuildBlock, 12 * static_cast<size_t>(S), s>>>(
            dev_src, sh, num_batches, batch_row, batch_tile, groups, meta, cells_t, a_val, a_lcol, a_drow, staged ? todo : nullptr);
        cell_padding_kernel<<<static_cast<int>(std::min<long long>((cells + kBlock - 1) / kBlock, 4096)), kBlock, 0, s>>>(
            cell_slots, offs, cells, a_val, a_lcol, a_drow);
    }
    e = hipGetLastError();
    out->host_strip.assign(S + 1, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(out->host_strip.data(), strip_begin, out->host_strip.size() * sizeof(int),
                                            hipMemcpyDeviceToHost, s);
    int pass_total = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&pass_total, pass_first + pass_waves, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    plan->num_passes = pass_total;
    trace.mark("allocations + placing (sync)");
    return hipSuccess;
}

} // namespace

hipError_t build_cells(const CSRMatrix* A, TiledPlan* plan, BuiltCells* out, hipStream_t s) {
    const CsrSource dev_src{A->d_row_ptrs, A->d_col_indices, A->d_values};
    return build_cells_from(dev_src, true, plan, out, s);
}

hipError_t build_cells(const ELLMatrix* A, TiledPlan* plan, BuiltCells* out, hipStream_t s) {
    const EllSource dev_src{A->num_rows, A->max_nnz_per_row, A->d_col_indices, A->d_values};
    return build_cells_from(dev_src, false, plan, out, s);
}

// phase 2's pass descriptors and pass-ordered row deltas (pass_layout_kernel; counted and scanned beside the placing
// pass in build_cells)
hipError_t layout_passes(TiledPlan* plan, hipStream_t s) {
    hipError_t e = dev_alloc(&plan->pass_desc, plan->num_passes);
    if (e == hipSuccess) e = dev_alloc(&plan->pass_word, 64 * plan->num_passes);
    if (e != hipSuccess) return e;
    pass_layout_kernel<true><<<plan->num_tiles, kReduceThreads, 0, s>>>(plan->num_tiles, plan->num_strips,
                                                                       reinterpret_cast<const int2*>(plan->cells_t.get()), plan->a_drow.get(), nullptr,
                                                                       plan->pass_first.get(), plan->pass_desc.get(), plan->pass_word.get());
    return hipGetLastError();
}

} // namespace detail
} // namespace spmv
