// tiled_build.hip — second half of the LDS-tiled engine's plan builder and its entry points (tiled.hip describes the
// engine and its layout): build_plan has tiled_cells.hip place the entries into cells, then cuts the long rows into
// chunks, probes whether the values fold into column weights and cuts the strips into phase-1 work items.
#include "tiled_build.h"
#include "tiled_layout.h"
#include "device_common.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxItemEntries = 16384;   // phase-1 work item size bounds (entries).  Round 4: 65536 -> 16384 — with the strip staging
                                         // pipelined, many short workgroups balance better than few long ones (C5 phase 1: 321.7 us with
                                         // ~53 K-slot items, 332.6 with 44 K (7.16 rounds of 512), 315.9 with 29 K, 315.2 with 22 K, 310.8-311.4 with
                                         // 15.5 K; on a faster box 296-300 / 290-295 (16 K) / 292-294 (12 K) / 308-311 (8 K))
constexpr int kMinItemEntries = 4096;
constexpr int kMaxLongRow = 4096;     // rows longer than min(this, 8 entries per strip) bypass the cells

// Column-weight folding: when every stored entry of a column carries the same value
// (adjacency matrices, the column-stochastic matrices of PageRank: a_ij = 1 / outdeg(j)),
// a_ij * x_j = (w_j * x_j) is one product per column instead of one per entry, and phase 1 no
// longer needs the value stream.  One workgroup per strip, the strip's weights in LDS: first every
// entry stores its value at its column, then every entry compares its bits with what stayed there.
// Skip markers / padding (row delta 255) carry no value.  Columns without an entry in the cells keep the
// kNoWeight bit pattern until the long rows have had their say (weight_finish_kernel turns what is left into 0).
constexpr unsigned int kNoWeight = 0x7FC0BEEFu;       // a NaN payload no arithmetic produces
template <int W>
__global__ __launch_bounds__(1024)
void strip_weight_kernel(int first_strip, int slot_limit, const int* __restrict__ strip_begin, int num_cols,
                         const float* __restrict__ a_val, const unsigned short* __restrict__ a_lcol,
                         const unsigned char* __restrict__ a_drow,
                         float* __restrict__ weight, int* __restrict__ differs) {
    __shared__ float ws[W];
    const int strip = first_strip + blockIdx.x;
    const int begin = strip_begin[strip];
    const int end = static_cast<int>(min(static_cast<long long>(strip_begin[strip + 1]), static_cast<long long>(begin) + slot_limit));
    for (int i = threadIdx.x; i < W; i += 1024) ws[i] = __uint_as_float(kNoWeight);
    __syncthreads();
    for (int q = begin + threadIdx.x; q < end; q += 1024) {
        if (a_drow[q] != kSkip) ws[a_lcol[q]] = a_val[q];
    }
    __syncthreads();
    bool bad = false;
    for (int q = begin + threadIdx.x; q < end; q += 1024) {
        if (a_drow[q] != kSkip) bad |= __float_as_uint(ws[a_lcol[q]]) != __float_as_uint(a_val[q]);
    }
    if (bad) *differs = 1;
    if (!weight) return;                 // sampling round: only the verdict is wanted
    const long long base = static_cast<long long>(strip) * W;
    for (int i = threadIdx.x; i < W && base + i < num_cols; i += 1024) weight[base + i] = ws[i];
}

// the long rows' entries are not in the cells: PASS 0 gives columns that only they touch a weight,
// PASS 1 checks that every long-row entry carries its column's weight
template <int PASS>
__global__ __launch_bounds__(kBlock)
void long_row_weight_kernel(const int* __restrict__ chunks, int num_chunks, const int* __restrict__ cols,
                            const float* __restrict__ vals, float* __restrict__ weight,
                            int* __restrict__ differs) {
    const int which = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (which >= num_chunks) return;
    bool bad = false;
    for (int j = chunks[3 * which + 1] + (threadIdx.x & 63); j < chunks[3 * which + 2]; j += 64) {
        unsigned int* slot = reinterpret_cast<unsigned int*>(weight + cols[j]);
        if (PASS == 0) {
            if (*slot == kNoWeight) atomicCAS(slot, kNoWeight, __float_as_uint(vals[j]));
        } else {
            bad |= *slot != __float_as_uint(vals[j]);
        }
    }
    if (PASS == 1 && bad) *differs = 1;
}

__global__ __launch_bounds__(kBlock)
void weight_finish_kernel(float* __restrict__ weight, int n) {
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        if (__float_as_uint(weight[i]) == kNoWeight) weight[i] = 0.0f;
    }
}

// The last step of the build on plans with strip_cols <= kPackedStripCols: the local columns, u16 per slot, into the
// 14-bit blocks phase 1 reads (tiled_layout.h).  One wavefront per block of 256 slots: lane l holds the slots
// 256 b + 4 l .. + 3 (zeros past the last slot), stores their low bytes as dword l of the low plane and hands its 24 high
// bits to the lanes that store the high field's 48 dwords — dword d is bits 32 d .. 32 d + 31 of the field, lane k's
// bits are 24 k .. 24 k + 23, so dword d takes the bits from 8 (4 d % 3) up of lane 4 d / 3 and the rest from the next lane.
__global__ __launch_bounds__(kBlock)
void pack_cols_kernel(long long slots, long long blocks, const unsigned short* __restrict__ a_lcol,
                      unsigned char* __restrict__ cols14) {
    const int lane = threadIdx.x & 63;
    for (long long b = static_cast<long long>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6); b < blocks;
         b += static_cast<long long>(gridDim.x) * (kBlock / 64)) {
        const long long q = b * kColBlockSlots + 4 * lane;
        unsigned int lo = 0, hi = 0;
        u16x4 mine = {0, 0, 0, 0};
        if (q + 3 < slots) {
            mine = *reinterpret_cast<const u16x4*>(a_lcol + q);
        } else {
            for (int e = 0; e < 4 && q + e < slots; ++e) mine[e] = a_lcol[q + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned int c = mine[e];
            lo |= (c & 0xFFu) << (8 * e);
            hi |= ((c >> 8) & 0x3Fu) << (6 * e);
        }
        unsigned char* block = cols14 + col_block_byte(q);
        reinterpret_cast<unsigned int*>(block)[lane] = lo;
        const int d = min(lane, 47);
        const int from = 4 * d / 3, off = 8 * (4 * d % 3);
        const unsigned int a = __shfl(hi, from, 64), next = __shfl(hi, from + 1, 64);
        if (lane < 48) reinterpret_cast<unsigned int*>(block + kColLowBytes)[lane] = (a >> off) | (next << (24 - off));
    }
}

// position-weighted checksums of the three slot streams and of the cell table (a debugging / test aid: two
// builds of one matrix must give the same four numbers whatever path the builder took).  The row deltas are summed
// where the finished plan keeps them: in pass order (pass_word), a function of the slots' bytes and the cell table alone.
// The local columns are decoded where the plan holds them packed (cols14): the same number as over the u16 array.
__global__ __launch_bounds__(kBlock)
void plan_checksum_kernel(long long slots, const float* __restrict__ a_val, const unsigned short* __restrict__ a_lcol,
                          const unsigned char* __restrict__ cols14,
                          long long delta_words, const unsigned int* __restrict__ pass_word,
                          long long table_ints, const int* __restrict__ cells_t,
                          unsigned long long* __restrict__ out /*[4]*/) {
    unsigned long long v = 0, c = 0, d = 0, t = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < slots;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const unsigned long long w = 2 * static_cast<unsigned long long>(i) + 1;
        if (a_val) v += w * __float_as_uint(a_val[i]);
        c += w * static_cast<unsigned long long>(lcol_at(a_lcol, cols14, i));
    }
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < delta_words;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        d += (2 * static_cast<unsigned long long>(i) + 1) * pass_word[i];
    }
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < table_ints;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        t += (2 * static_cast<unsigned long long>(i) + 1) * static_cast<unsigned int>(cells_t[i]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_xor(v, off, 64);
        c += __shfl_xor(c, off, 64);
        d += __shfl_xor(d, off, 64);
        t += __shfl_xor(t, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], v);
        atomicAdd(&out[1], c);
        atomicAdd(&out[2], d);
        atomicAdd(&out[3], t);
    }
}

// where the entries come from: exactly one of csr / ell is set
struct Source {
    const CSRMatrix* csr = nullptr;
    const ELLMatrix* ell = nullptr;
    int rows = 0, cols = 0;
    long long nnz = 0;        // CSR: exact; ELL: slots (upper bound, used for shape / capacity only)
};

// cuts the long rows into wavefront-sized chunks (the list is short: <= nnz / long_row rows)
hipError_t cut_long_rows(const CSRMatrix* A, TiledPlan* plan) {
    std::vector<int> rows(plan->num_long);
    hipError_t e = hipMemcpy(rows.data(), plan->long_rows.get(), rows.size() * sizeof(int), hipMemcpyDeviceToHost);
    std::sort(rows.begin(), rows.end());           // the device listed them in arrival order
    if (e == hipSuccess) e = hipMemcpy(plan->long_rows.get(), rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice);
    std::vector<int> chunks;
    std::vector<int> all_ptrs;                       // many long rows: one bulk copy instead
    const int* host_ptrs = A->row_ptrs;
    if (!host_ptrs && plan->num_long > 256 && e == hipSuccess) {
        all_ptrs.resize(static_cast<size_t>(A->num_rows) + 1);
        e = hipMemcpy(all_ptrs.data(), A->d_row_ptrs, all_ptrs.size() * sizeof(int), hipMemcpyDeviceToHost);
        host_ptrs = all_ptrs.data();
    }
    std::vector<int> first_chunk;
    for (int row : rows) {
        first_chunk.push_back(static_cast<int>(chunks.size() / 3));
        int span[2] = {0, 0};
        if (host_ptrs) {
            span[0] = host_ptrs[row];
            span[1] = host_ptrs[row + 1];
        } else if (e == hipSuccess) {
            e = hipMemcpy(span, A->d_row_ptrs + row, sizeof(span), hipMemcpyDeviceToHost);
        }
        for (int b = span[0]; e == hipSuccess && b < span[1]; b += kLongChunk) {
            chunks.push_back(row);
            chunks.push_back(b);
            chunks.push_back(std::min(b + kLongChunk, span[1]));
        }
    }
    plan->num_long_chunks = static_cast<int>(chunks.size() / 3);
    first_chunk.push_back(plan->num_long_chunks);
    if (e == hipSuccess) e = dev_alloc(&plan->long_first, static_cast<long long>(first_chunk.size()));
    if (e == hipSuccess) e = hipMemcpy(plan->long_first.get(), first_chunk.data(), first_chunk.size() * sizeof(int),
                                       hipMemcpyHostToDevice);
    if (e == hipSuccess) e = dev_alloc(&plan->long_sums, plan->num_long_chunks);
    if (e == hipSuccess) e = dev_alloc(&plan->long_chunks, static_cast<long long>(chunks.size()));
    if (e == hipSuccess) e = hipMemcpy(plan->long_chunks.get(), chunks.data(), chunks.size() * sizeof(int),
                                       hipMemcpyHostToDevice);
    if (e == hipSuccess) {          // first long row of every tile (the list is ascending)
        std::vector<int> tile_long(static_cast<size_t>(plan->num_tiles) + 1);
        size_t at = 0;
        for (int t = 0; t <= plan->num_tiles; ++t) {
            const long long bound = static_cast<long long>(t) * plan->tile_rows;
            while (at < rows.size() && rows[at] < bound) ++at;
            tile_long[t] = static_cast<int>(at);
        }
        e = dev_alloc(&plan->tile_long, static_cast<long long>(tile_long.size()));
        if (e == hipSuccess) e = hipMemcpy(plan->tile_long.get(), tile_long.data(), tile_long.size() * sizeof(int),
                                           hipMemcpyHostToDevice);
    }
    return e;
}

// column-weight folding (see strip_weight_kernel).  The first few strips alone settle it for arbitrary values (a
// column that occurs twice there already differs).  Leaves the plan with either a_val or col_weight.
hipError_t probe_fold(TiledPlan* plan, const int* strip_begin, hipStream_t s) {
    DevBuf<int> differs;
    hipError_t e = dev_alloc(&differs, 1);
    if (e == hipSuccess) e = hipMemsetAsync(differs.get(), 0, sizeof(int), s);
    int host_differs = 1;
    auto probe = [&](int first, int count, int limit, float* weight) {
        with_strip_width(plan->strip_cols, [&](auto width) {
            strip_weight_kernel<decltype(width)::value><<<count, 1024, 0, s>>>(
                first, limit, strip_begin, plan->num_cols, plan->a_val.get(), plan->a_lcol.get(), plan->a_drow.get(), weight, differs.get());
        });
    };
    // round 0: the first 32 K slots of up to 64 strips, verdict only (with arbitrary values some column
    // repeats there and the matter is settled before anything is allocated); round 1: everything
    const int sample = std::min(plan->num_strips, 64);
    for (int round = 0; round < 2 && e == hipSuccess; ++round) {
        if (round == 0) {
            probe(0, sample, 32768, nullptr);
        } else {
            e = dev_alloc(&plan->col_weight, plan->num_cols);
            if (e != hipSuccess) break;
            float* weight = plan->col_weight.get();
            probe(0, plan->num_strips, 0x7fffffff, weight);
            if (plan->num_long_chunks > 0) {
                const int grid = (plan->num_long_chunks + kBlock / 64 - 1) / (kBlock / 64);
                long_row_weight_kernel<0><<<grid, kBlock, 0, s>>>(plan->long_chunks.get(), plan->num_long_chunks, plan->csr_cols,
                                                               plan->csr_vals, weight, differs.get());
                long_row_weight_kernel<1><<<grid, kBlock, 0, s>>>(plan->long_chunks.get(), plan->num_long_chunks, plan->csr_cols,
                                                               plan->csr_vals, weight, differs.get());
            }
            weight_finish_kernel<<<std::min(2048, (plan->num_cols + kBlock - 1) / kBlock), kBlock, 0, s>>>(weight, plan->num_cols);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&host_differs, differs.get(), sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (host_differs) break;
    }
    if (e != hipSuccess) return e;
    if (host_differs) {
        plan->col_weight.reset();
    } else {
        plan->a_val.reset();           // folded: phase 1 reads weights, not values
    }
    return hipSuccess;
}

// phase-1 work items: every strip's range cut into EQUAL pieces of <= item_entries (enough
// pieces to fill the chip several times), piece boundaries on multiples of 8 slots
hipError_t make_items(TiledPlan* plan, const std::vector<int>& host_strip) {
    const long long floor_entries = std::max<long long>(kMinItemEntries, plan->strip_cols);   // strip load <= 40 % of the stream
    // (a folded plan stages TWO arrays per item — x and the column weights — and streams 6 bytes per slot instead of 10:
    // 16 K-slot items cost it 12 %, 0.460 against 0.41 ms per PageRank step on C5; it keeps the larger items)
    const long long item_cap = plan->col_weight ? 4 * kMaxItemEntries : kMaxItemEntries;
    int item_entries = static_cast<int>(std::max<long long>(
        floor_entries, std::min<long long>(item_cap, (plan->nnz / 2048 + 7) / 8 * 8)));
    item_entries = static_cast<int>(std::max(1024LL, debug_number("item", item_entries)));
    std::vector<int> items;
    plan->strip_first_item.assign(static_cast<size_t>(plan->num_strips) + 1, 0);
    for (int strip = 0; strip < plan->num_strips; ++strip) {
        plan->strip_first_item[strip] = static_cast<int>(items.size() / 3);
        const int begin = host_strip[strip], stop = host_strip[strip + 1];
        const int parts = (stop - begin + item_entries - 1) / item_entries;
        int b = begin;
        for (int part = 1; part <= parts; ++part) {
            int next = part == parts ? stop
                                     : static_cast<int>(begin + static_cast<long long>(stop - begin) * part / parts) / 8 * 8;
            next = std::max(next, b);
            if (next == b && part != parts) continue;
            items.push_back(strip);
            items.push_back(b);
            items.push_back(next);
            b = next;
        }
    }
    plan->num_items = static_cast<int>(items.size() / 3);
    plan->strip_first_item[plan->num_strips] = plan->num_items;
    hipError_t e = dev_alloc(&plan->items, static_cast<long long>(items.size()));
    if (e == hipSuccess && !items.empty()) {
        e = hipMemcpy(plan->items.get(), items.data(), items.size() * sizeof(int), hipMemcpyHostToDevice);
    }
    return e;
}

hipError_t build_plan(const Source& src, TiledPlan** out, hipStream_t s) {
    const auto t_begin = std::chrono::steady_clock::now();
    BuildTrace trace;
    const CSRMatrix* A = src.csr;          // null for an ELL source (then no long-row path)
    *out = nullptr;
    std::unique_ptr<TiledPlan, decltype(&tiled_free)> plan(new TiledPlan(), &tiled_free);     // the caller's on success only
    plan->num_rows = src.rows;
    plan->num_cols = src.cols;
    plan->csr_nnz = src.nnz;
    if (A) {
        plan->csr_row_ptrs = A->d_row_ptrs;
        plan->csr_cols = A->d_col_indices;
        plan->csr_vals = A->d_values;
    } else {
        plan->csr_vals = src.ell->d_values;       // identity of the slabs the plan was built from (aux_table.cpp)
    }
    choose_shape(src.rows, src.cols, src.nnz, &plan->strip_cols, &plan->tile_rows);
    plan->num_strips = (src.cols + plan->strip_cols - 1) / plan->strip_cols;
    plan->num_tiles = (src.rows + plan->tile_rows - 1) / plan->tile_rows;
    const long long cells = static_cast<long long>(plan->num_strips) * plan->num_tiles;
    // A row spreads over the strips; rows with many entries per cell make lanes meet on one LDS word in phase 2,
    // so the longest rows take the direct path instead (512-entry chunks, direct gather, seeds).  With the
    // compare-and-swap add of round 1 the line sat at 2-4 entries per strip; the hardware ds_add_f64 takes
    // collisions far better (profiles/r02_long_row_sweep.txt, C4 = 1 M power-law rows, 62 strips: limit 124
    // entries 49.5 us, 248: 47.2, 496: 44.2, unlimited 47.8; 10 M x 10 M power-law: 426 / 435 / 416 / 402 us).
    int long_factor = 8;
    long_factor = static_cast<int>(std::max(1LL, debug_number("long_factor", long_factor)));
    int long_cap = kMaxLongRow;
    long_cap = static_cast<int>(std::max(64LL, debug_number("long_cap", long_cap)));
    plan->long_row = A ? std::max(64, std::min(long_cap, long_factor * plan->num_strips)) : 0x3fffffff;

    bool fold = true;          // on unless SPMV_TILED_FOLD=0
    if (const char* env = std::getenv("SPMV_TILED_FOLD")) fold = env[0] != '0';
    BuiltCells built;
    hipError_t e = A ? build_cells(A, plan.get(), &built, s) : build_cells(src.ell, plan.get(), &built, s);
    trace.mark("cells built, temporaries freed");
    if (e == hipSuccess) e = layout_passes(plan.get(), s);
    if (e != hipSuccess) return e;
    trace.mark("phase-2 pass descriptors");

    if (A && plan->num_long > 0) e = cut_long_rows(A, plan.get());
    if (e == hipSuccess && fold && plan->nnz > 0) e = probe_fold(plan.get(), built.strip_begin.get(), s);
    if (e != hipSuccess) return e;
    built.strip_begin.reset();
    // The slot-ordered row deltas have served (pass layout, fold probe): phase 2 reads the pass-ordered copy.  The free
    // waits for the device, like the temporaries' above.
    plan->a_drow.reset();

    e = dev_alloc(&plan->prod, plan->nnz + 8);
    if (e == hipSuccess) e = make_items(plan.get(), built.host_strip);
    if (e != hipSuccess) return e;
    trace.mark("fold probe, long rows, items");

    // The local columns have served as u16 (placing passes, fold probe): phase 1 reads them packed to 14 bits wherever a
    // strip has no more than 16384 columns (tiled_layout.h).  SPMV_DEBUG=cols=u16 keeps the u16 array: the A/B switch.
    if (plan->strip_cols <= kPackedStripCols && plan->nnz > 0 && !debug_is("cols", "u16")) {
        const long long blocks = (plan->nnz + kColBlockSlots - 1) / kColBlockSlots;
        e = dev_alloc(&plan->a_cols14, packed_col_bytes(plan->nnz));
        if (e != hipSuccess) return e;
        // (the slack behind the last block is only ever loaded, never used: cleared so that no run reads unwritten memory)
        e = hipMemsetAsync(plan->a_cols14.get() + blocks * kColBlockBytes, 0, kColSlackBytes, s);
        if (e != hipSuccess) return e;
        const int grid = static_cast<int>(std::min<long long>((blocks + kBlock / 64 - 1) / (kBlock / 64), 1 << 16));
        pack_cols_kernel<<<grid, kBlock, 0, s>>>(plan->nnz, blocks, plan->a_lcol.get(), plan->a_cols14.get());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        plan->a_lcol.reset();
        trace.mark("local columns packed");
    }
    // plan_bytes keeps its accounting, two bytes of local column per slot: the tests' host model of the plan
    // (tests/tiled_model.py) holds the builder to that number.  For a packed plan it is an upper bound; col_bytes is
    // what the plan holds of columns, so its footprint is plan_bytes - 2 * nnz + col_bytes.
    plan->col_bytes = plan->a_cols14 ? packed_col_bytes(plan->nnz) : 2 * plan->nnz;
    plan->plan_bytes = plan->nnz * (4 /*prod*/ + 2 + (plan->a_val ? 4 : 0)) + cells * 8 +
                       plan->num_passes * static_cast<long long>(sizeof(PassDesc) + kPassSlots /*pass_word*/) +
                       4LL * (plan->num_tiles * kReduceWaves + 1) +
                       (plan->col_weight ? 4LL * plan->num_cols : 0) +
                       12LL * plan->num_items + 12LL * plan->num_long_chunks;
    plan->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    *out = plan.release();
    return hipSuccess;
}

} // namespace

hipError_t tiled_build(const CSRMatrix* A, TiledPlan** out, hipStream_t s) {
    Source src;
    src.csr = A;
    src.rows = A->num_rows;
    src.cols = A->num_cols;
    src.nnz = A->nnz;
    return build_plan(src, out, s);
}

hipError_t tiled_build(const ELLMatrix* A, TiledPlan** out, hipStream_t s) {
    Source src;
    src.ell = A;
    src.rows = A->num_rows;
    src.cols = A->num_cols;
    src.nnz = static_cast<long long>(A->num_rows) * A->max_nnz_per_row;
    return build_plan(src, out, s);
}


void tiled_free(TiledPlan* p) { delete p; }

hipError_t tiled_checksum(const TiledPlan& plan, unsigned long long out[4], hipStream_t s) {
    DevBuf<unsigned long long> d_out;
    hipError_t e = dev_alloc(&d_out, 4);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(d_out.get(), 0, 4 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        plan_checksum_kernel<<<1024, kBlock, 0, s>>>(plan.nnz, plan.a_val.get(), plan.a_lcol.get(), plan.a_cols14.get(), 64 * plan.num_passes,
                                                     plan.pass_word.get(), 2LL * plan.num_strips * plan.num_tiles,
                                                     plan.cells_t.get(), d_out.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.get(), 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

} // namespace detail
} // namespace spmv
