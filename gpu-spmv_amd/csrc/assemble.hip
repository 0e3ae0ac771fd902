// assemble.hip — device matrix assembly (include/spmv/assemble.h): CSR from unsorted triplets with
// repeats, bit for bit csr_from_coo_cpu's result, and the one-launch refill of its values.  No atomics of any kind.
//
//   validate    one kernel over the triplets: every row in [0, num_rows), every column in [0, num_cols); per workgroup
//               a flag and the OR of (key ^ key[0]), key = (row << col_bits) | col — digits whose bits never differ
//               are constant and their passes are skipped.  The host reads these before anything else is allocated.
//   per pass    a stable LSD radix pass on an 8-bit digit over (key, source position); the key is a 32-bit integer
//               when it fits and a 64-bit one otherwise.  The first pass forms its keys from the caller's arrays.
//                 count    digit counts per tile of kTileEntries entries by wavefront matching, stored digit-major
//                 scan     detail::device_exclusive_scan of the counts
//                 scatter  a wavefront ranks 16 rounds of 64 consecutive entries against per-wavefront digit counters
//                          in LDS and keeps (key, position, rank) in registers; one scan over the 256 digits turns the
//                          counters into the tile's digit-ordered layout; the tile is written into LDS in that order;
//                          then consecutive lanes copy consecutive LDS slots to global memory, so every digit's run
//                          leaves as one contiguous piece instead of 64 separate 4-byte stores.
//   compress    head flags key[t] != key[t-1], their exclusive scan, one read of nnz_out; then C's columns, the
//               segment starts and the row pointers (a lower bound over the sorted keys per row).  COO_KEEP has no
//               flags: every entry is a head.
//   numeric     one thread per output entry adds its segment left to right (ascending sorted slot = ascending source
//               position: the sort is stable).  The same kernel is csr_coo_refill.
#include "assemble_impl.h"
#include "internal.h"
#include "device_common.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace spmv {
namespace detail {
namespace assemble {

namespace {

using dev::kBlock;
using dev::vec_grid;

constexpr int kWaves = kSortThreads / 64;
constexpr int kWaveChunk = kTileEntries / kWaves;     // consecutive entries one wavefront ranks
constexpr int kValidateGrid = 2048;

__device__ __forceinline__ unsigned lanes_below(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0u));
}

// lanes of this wavefront that hold a valid entry with the same 8-bit digit as this lane
__device__ __forceinline__ unsigned long long match_digit(bool valid, unsigned digit) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long set = __ballot(bit);
        m &= bit ? set : ~set;
    }
    return m;
}

// the lanes of one wavefront hand values to each other through LDS between two of these
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename K>
__device__ __forceinline__ K make_key(int row, int col, int col_bits) {
    return (static_cast<K>(static_cast<unsigned>(row)) << col_bits) | static_cast<K>(static_cast<unsigned>(col));
}

template <typename K>
__device__ __forceinline__ unsigned digit_of(K key, int shift) {
    return static_cast<unsigned>(key >> shift) & 255u;
}

// what a pass reads: the caller's triplets (the first pass; position = index) or the previous pass's output
template <typename K>
struct SortInput {
    const int* rows;
    const int* cols;
    int col_bits;
    const K* keys;
    const int* pos;
};

template <typename K, bool kFirst>
__device__ __forceinline__ void load_entry(const SortInput<K>& in, long long i, K* key, int* pos) {
    if constexpr (kFirst) {
        *key = make_key<K>(in.rows[i], in.cols[i], in.col_bits);
        *pos = static_cast<int>(i);
    } else {
        *key = in.keys[i];
        *pos = in.pos[i];
    }
}

// ---- validation: partial[3b] = violation seen by workgroup b, partial[3b+1], [3b+2] = OR of (key ^ key[0]) ----
__global__ __launch_bounds__(kBlock) void assemble_validate_kernel(const int* __restrict__ rows,
                                                                   const int* __restrict__ cols, int n, int num_rows,
                                                                   int num_cols, int col_bits,
                                                                   unsigned* __restrict__ partial) {
    __shared__ int s_bad[kBlock / 64];
    __shared__ unsigned s_lo[kBlock / 64], s_hi[kBlock / 64];
    const unsigned long long ref = make_key<unsigned long long>(rows[0], cols[0], col_bits);
    bool bad = false;
    unsigned long long diff = 0;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int r = rows[i], c = cols[i];
        if (r < 0 || r >= num_rows || c < 0 || c >= num_cols) bad = true;
        diff |= make_key<unsigned long long>(r, c, col_bits) ^ ref;
    }
    unsigned lo = static_cast<unsigned>(diff), hi = static_cast<unsigned>(diff >> 32);
    for (int off = 32; off > 0; off >>= 1) {
        lo |= __shfl_xor(lo, off, 64);
        hi |= __shfl_xor(hi, off, 64);
    }
    const unsigned long long any_bad = __ballot(bad);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_bad[wave] = any_bad != 0;
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned b = 0, l = 0, h = 0;
        for (int w = 0; w < kBlock / 64; ++w) {
            b |= static_cast<unsigned>(s_bad[w]);
            l |= s_lo[w];
            h |= s_hi[w];
        }
        partial[3 * blockIdx.x] = b;
        partial[3 * blockIdx.x + 1] = l;
        partial[3 * blockIdx.x + 2] = h;
    }
}

// no pass at all (every key equal): the keys and the identity order
template <typename K>
__global__ __launch_bounds__(kBlock) void assemble_keys_kernel(SortInput<K> in, int n, K* __restrict__ keys,
                                                               int* __restrict__ pos) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        load_entry<K, true>(in, i, &keys[i], &pos[i]);
    }
}

// counts[d * num_tiles + t] = entries of tile t whose digit is d
template <typename K, bool kFirst>
__global__ __launch_bounds__(kSortThreads) void assemble_count_kernel(SortInput<K> in, int n, int shift,
                                                                      int num_tiles, int* __restrict__ counts) {
    __shared__ int s_cnt[kWaves][256];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const long long tile = blockIdx.x * static_cast<long long>(kTileEntries);
    for (int r = 0; r < kSortRounds; ++r) {
        const long long i = tile + r * kSortThreads + threadIdx.x;
        const bool valid = i < n;
        K key = 0;
        int pos = 0;
        if (valid) load_entry<K, kFirst>(in, i, &key, &pos);
        const unsigned d = digit_of(key, shift);
        const unsigned long long m = match_digit(valid, d);
        // the highest lane of each digit group adds the group's size: one writer per (wavefront, digit)
        if (valid && lanes_below(m) == static_cast<unsigned>(__popcll(m)) - 1) s_cnt[wave][d] += __popcll(m);
        wave_sync();
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += s_cnt[w][threadIdx.x];
    counts[static_cast<long long>(threadIdx.x) * num_tiles + blockIdx.x] = total;
}

// Stable scatter of one pass through an LDS image of the tile.  offsets[d * num_tiles + t] = where tile t's first
// digit-d entry goes.  Wavefront w ranks the entries [w * kWaveChunk, (w + 1) * kWaveChunk) of the tile, 64
// consecutive ones per round, so tile order is (wavefront, round, lane) order.
template <typename K, bool kFirst>
__global__ __launch_bounds__(kSortThreads) void assemble_scatter_kernel(SortInput<K> in, int n, int shift,
                                                                        int num_tiles,
                                                                        const int* __restrict__ offsets,
                                                                        K* __restrict__ keys_out,
                                                                        int* __restrict__ pos_out) {
    __shared__ K s_key[kTileEntries];
    __shared__ int s_pos[kTileEntries];
    __shared__ int s_cnt[kWaves][256];       // per (wavefront, digit): entries seen, then first LDS slot
    __shared__ int s_global[256];            // per digit: global position of LDS slot 0, were the run to start there
    __shared__ int s_wave_total[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();

    // ---- rank: after this s_cnt[wave][d] counts the wavefront's digit-d entries, rank[r] those before entry r ----
    const long long tile = blockIdx.x * static_cast<long long>(kTileEntries);
    const long long chunk = tile + wave * kWaveChunk;
    K key[kSortRounds];
    int pos[kSortRounds];
    int rank[kSortRounds];
    // (all of the wavefront's loads are issued before the first round waits for one)
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const long long i = chunk + r * 64 + lane;
        key[r] = 0;
        pos[r] = 0;
        if (i < n) load_entry<K, kFirst>(in, i, &key[r], &pos[r]);
    }
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const bool valid = chunk + r * 64 + lane < n;
        const unsigned d = digit_of(key[r], shift);
        const unsigned long long m = match_digit(valid, d);
        const int below = static_cast<int>(lanes_below(m));
        const int before = s_cnt[wave][d];
        rank[r] = before + below;
        wave_sync();
        if (valid && below == __popcll(m) - 1) s_cnt[wave][d] = before + below + 1;
        wave_sync();
    }
    __syncthreads();

    // ---- layout: thread d turns the counters of digit d into first slots; digits in ascending order ----
    {
        int c[kWaves];
        int total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            c[w] = s_cnt[w][threadIdx.x];
            total += c[w];
        }
        const int inclusive = dev::wave_inclusive_scan(total);
        if (lane == 63) s_wave_total[wave] = inclusive;
        __syncthreads();
        int start = inclusive - total;
        for (int w = 0; w < wave; ++w) start += s_wave_total[w];
        s_global[threadIdx.x] = offsets[static_cast<long long>(threadIdx.x) * num_tiles + blockIdx.x] - start;
        int run = start;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            s_cnt[w][threadIdx.x] = run;
            run += c[w];
        }
    }
    __syncthreads();

    // ---- the tile in digit order, in LDS ----
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        if (chunk + r * 64 + lane < n) {
            const int slot = s_cnt[wave][digit_of(key[r], shift)] + rank[r];
            s_key[slot] = key[r];
            s_pos[slot] = pos[r];
        }
    }
    __syncthreads();

    // ---- out: consecutive lanes, consecutive slots, consecutive addresses within a digit's run ----
    const int held = static_cast<int>(std::min<long long>(kTileEntries, n - tile));
    for (int j = threadIdx.x; j < held; j += kSortThreads) {
        const K k = s_key[j];
        const int where = s_global[digit_of(k, shift)] + j;
        keys_out[where] = k;
        pos_out[where] = s_pos[j];
    }
}

// flags[t] = 1 where sorted slot t begins an entry, for t < n; flags[n] = 0 (its scan is nnz_out)
template <typename K>
__global__ __launch_bounds__(kBlock) void assemble_heads_kernel(const K* __restrict__ keys, int n,
                                                                int* __restrict__ flags) {
    for (long long t = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; t <= n;
         t += static_cast<long long>(gridDim.x) * kBlock) {
        flags[t] = t < n && (t == 0 || keys[t] != keys[t - 1]);
    }
}

// the columns and the segment starts; index = the scanned flags, or null when every slot is an entry (COO_KEEP)
template <typename K>
__global__ __launch_bounds__(kBlock) void assemble_entries_kernel(const K* __restrict__ keys, int n,
                                                                  const int* __restrict__ index, K col_mask,
                                                                  int nnz_out, int* __restrict__ col_out,
                                                                  int* __restrict__ segments) {
    for (long long t = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; t < n;
         t += static_cast<long long>(gridDim.x) * kBlock) {
        const K k = keys[t];
        if (!index) {
            col_out[t] = static_cast<int>(k & col_mask);
        } else if (t == 0 || k != keys[t - 1]) {
            const int o = index[t];
            col_out[o] = static_cast<int>(k & col_mask);
            segments[o] = static_cast<int>(t);
        }
        if (t == 0 && segments) segments[nnz_out] = n;
    }
}

// row_ptrs[r] = output entries with row < r, for r in [0, num_rows]: the lower bound of r's first key
template <typename K>
__global__ __launch_bounds__(kBlock) void assemble_row_ptrs_kernel(const K* __restrict__ keys, int n,
                                                                   const int* __restrict__ index, int num_rows,
                                                                   int col_bits, int* __restrict__ row_ptrs) {
    const long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x;
    if (r > num_rows) return;
    const unsigned long long first = static_cast<unsigned long long>(r) << col_bits;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (static_cast<unsigned long long>(keys[mid]) < first) lo = mid + 1; else hi = mid;
    }
    row_ptrs[r] = index ? index[lo] : lo;      // index[n] = nnz_out
}

// values[o] = vals[order[t0]] + vals[order[t0 + 1]] + ... left to right over the entry's segment; a lone value is
// copied, and the NaN of an addition has one spelling (assemble.h)
__global__ __launch_bounds__(kBlock) void assemble_numeric_kernel(const int* __restrict__ order,
                                                                  const int* __restrict__ segments,
                                                                  const float* __restrict__ vals, int nnz_out,
                                                                  float* __restrict__ values) {
    for (long long o = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; o < nnz_out;
         o += static_cast<long long>(gridDim.x) * kBlock) {
        if (!segments) {
            values[o] = vals[order[o]];
            continue;
        }
        const int begin = segments[o], end = segments[o + 1];
        float s = vals[order[begin]];
        for (int t = begin + 1; t < end; ++t) s += vals[order[t]];
        if (end - begin > 1 && s != s) s = __builtin_bit_cast(float, 0x7FC00000u);
        values[o] = s;
    }
}

struct Request {
    int num_rows, num_cols, n;
    const int* d_rows;
    const int* d_cols;
    const float* d_vals;
    int duplicates;
};

// the sort, the compression and the values for keys of type K; `diff` = OR of (key ^ key[0]) over all triplets
template <typename K>
int build_sorted(CSRMatrix* C, const Request& q, const KeyLayout& layout, unsigned long long diff, CooPlan** plan,
                 CooResult* result, hipStream_t s) {
    const int n = q.n;
    std::vector<int> shifts;
    for (int d = 0; 8 * d < layout.total_bits; ++d) {
        if ((diff >> (8 * d)) & 255u) shifts.push_back(8 * d);
    }
    const int passes = static_cast<int>(shifts.size());
    const int tiles = (n + kTileEntries - 1) / kTileEntries;
    const std::vector<long long> levels = device_scan_levels(256LL * tiles);

    DevBuf<K> keys[2];
    DevBuf<int> pos[2], counts;
    bool got = dev_alloc(&keys[0], n) == hipSuccess && dev_alloc(&pos[0], n) == hipSuccess;
    if (passes >= 2) got = got && dev_alloc(&keys[1], n) == hipSuccess && dev_alloc(&pos[1], n) == hipSuccess;
    if (passes >= 1) got = got && dev_alloc(&counts, 256LL * tiles + device_scan_sums(levels)) == hipSuccess;
    if (!got) return fail(result, SpMVError::CUDA_MALLOC);

    SortInput<K> in{q.d_rows, q.d_cols, layout.col_bits, nullptr, nullptr};
    bool ok = true;
    int cur = 0;
    if (passes == 0) {
        assemble_keys_kernel<K><<<vec_grid(n), kBlock, 0, s>>>(in, n, keys[0].get(), pos[0].get());
        ok = hipGetLastError() == hipSuccess;
        ++result->launches;
    }
    for (int j = 0; j < passes && ok; ++j) {
        cur = j % 2;
        const int shift = shifts[j];
        if (j == 0) {
            assemble_count_kernel<K, true><<<tiles, kSortThreads, 0, s>>>(in, n, shift, tiles, counts.get());
        } else {
            assemble_count_kernel<K, false><<<tiles, kSortThreads, 0, s>>>(in, n, shift, tiles, counts.get());
        }
        ok = hipGetLastError() == hipSuccess &&
             device_exclusive_scan(counts.get(), levels, counts.get() + levels[0], s) == hipSuccess;
        if (!ok) break;
        if (j == 0) {
            assemble_scatter_kernel<K, true><<<tiles, kSortThreads, 0, s>>>(in, n, shift, tiles, counts.get(),
                                                                            keys[cur].get(), pos[cur].get());
        } else {
            assemble_scatter_kernel<K, false><<<tiles, kSortThreads, 0, s>>>(in, n, shift, tiles, counts.get(),
                                                                             keys[cur].get(), pos[cur].get());
        }
        ok = hipGetLastError() == hipSuccess;
        result->launches += 2 + device_scan_launches(levels);
        in.keys = keys[cur].get();
        in.pos = pos[cur].get();
    }
    if (!ok) {
        (void)hipStreamSynchronize(s);
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    const K* sorted = keys[cur].get();

    // ---- compress: the one read of nnz_out ----
    int nnz_out = n;
    DevBuf<int> index, index_sums;
    const bool sum = q.duplicates == COO_SUM;
    if (sum) {
        const std::vector<long long> index_levels = device_scan_levels(static_cast<long long>(n) + 1);
        if (dev_alloc(&index, static_cast<long long>(n) + 1) != hipSuccess ||
            dev_alloc(&index_sums, device_scan_sums(index_levels)) != hipSuccess) {
            (void)hipStreamSynchronize(s);
            return fail(result, SpMVError::CUDA_MALLOC);
        }
        assemble_heads_kernel<K><<<vec_grid(static_cast<long long>(n) + 1), kBlock, 0, s>>>(sorted, n, index.get());
        ok = hipGetLastError() == hipSuccess &&
             device_exclusive_scan(index.get(), index_levels, index_sums.get(), s) == hipSuccess &&
             hipMemcpyAsync(&nnz_out, index.get() + n, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        result->launches += 1 + device_scan_launches(index_levels);
        if (!ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    }

    // ---- C's arrays and the plan's ----
    DeviceCsrArrays out;                // (nnz_out >= 1: there is a triplet)
    const ReleaseOnExit release_out{&out};
    DevBuf<int> segments;
    if (out.alloc(static_cast<long long>(q.num_rows) + 1, nnz_out) != hipSuccess ||
        (sum && dev_alloc(&segments, static_cast<long long>(nnz_out) + 1) != hipSuccess)) {
        (void)hipStreamSynchronize(s);
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    CooPlan* made = plan ? new CooPlan() : nullptr;
    const K col_mask = (static_cast<K>(1) << layout.col_bits) - 1;
    assemble_entries_kernel<K><<<vec_grid(n), kBlock, 0, s>>>(sorted, n, index.get(), col_mask, nnz_out,
                                                            out.col_indices, segments.get());
    assemble_row_ptrs_kernel<K><<<dev::capped_grid(static_cast<long long>(q.num_rows) + 1, kBlock, 1 << 23), kBlock, 0,
                                  s>>>(sorted, n, index.get(), q.num_rows, layout.col_bits, out.row_ptrs);
    assemble_numeric_kernel<<<vec_grid(nnz_out), kBlock, 0, s>>>(pos[cur].get(), segments.get(), q.d_vals, nnz_out,
                                                                 out.values);
    ok = hipGetLastError() == hipSuccess;
    result->launches += 3;
    EventPair& ev = thread_events();
    ok = ok && hipEventRecord(ev.stop, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok || hipEventElapsedTime(&result->elapsed_ms, ev.start, ev.stop) != hipSuccess) {
        delete made;
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    csr_adopt_device(C, q.num_rows, q.num_cols, nnz_out, &out);          // C owns them now
    if (made) {
        made->num_rows = q.num_rows;
        made->num_cols = q.num_cols;
        made->n = n;
        made->nnz_out = nnz_out;
        made->duplicates = q.duplicates;
        made->d_order = pos[cur].release();
        made->d_segments = segments.release();
        *plan = made;
    }
    result->nnz_out = nnz_out;
    result->combined = n - nnz_out;
    result->passes = passes;
    return 0;
}

// no triplets: an all-zero row_ptrs
int build_empty(CSRMatrix* C, const Request& q, CooPlan** plan, CooResult* result, hipStream_t s) {
    DeviceCsrArrays out;
    const ReleaseOnExit release_out{&out};
    DevBuf<int> segments;
    const size_t ptr_bytes = (static_cast<size_t>(q.num_rows) + 1) * sizeof(int);
    const bool sum = q.duplicates == COO_SUM;
    if (out.alloc(static_cast<long long>(q.num_rows) + 1, 0) != hipSuccess ||
        (plan && sum && dev_alloc(&segments, 1) != hipSuccess)) {
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    if (hipMemsetAsync(out.row_ptrs, 0, ptr_bytes, s) != hipSuccess ||
        (segments && hipMemsetAsync(segments.get(), 0, sizeof(int), s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess) {
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    csr_adopt_device(C, q.num_rows, q.num_cols, 0, &out);
    if (plan) {
        CooPlan* made = new CooPlan();
        made->num_rows = q.num_rows;
        made->num_cols = q.num_cols;
        made->duplicates = q.duplicates;
        made->d_segments = segments.release();
        *plan = made;
    }
    return 0;
}

int build(CSRMatrix* C, const Request& q, CooPlan** plan, CooResult* result, hipStream_t s) {
    const TraceRange range("spmv:csr_from_coo_gpu");
    if (q.n == 0) return build_empty(C, q, plan, result, s);

    // ---- validation: one kernel, one read of its per-workgroup words, before anything else is allocated ----
    const KeyLayout layout = key_layout(q.num_rows, q.num_cols);
    const int grid = dev::capped_grid(q.n, kBlock, kValidateGrid);
    DevBuf<unsigned> d_partial;
    if (dev_alloc(&d_partial, 3LL * grid) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    std::vector<unsigned> partial(3 * static_cast<size_t>(grid));
    EventPair& ev = thread_events();
    if (!ev.start || !ev.stop || hipEventRecord(ev.start, s) != hipSuccess) {
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    assemble_validate_kernel<<<grid, kBlock, 0, s>>>(q.d_rows, q.d_cols, q.n, q.num_rows, q.num_cols, layout.col_bits,
                                                     d_partial.get());
    bool ok = hipGetLastError() == hipSuccess &&
              hipMemcpyAsync(partial.data(), d_partial.get(), partial.size() * sizeof(unsigned),
                             hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    d_partial.reset();
    if (!ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    result->launches = 1;
    unsigned long long diff = 0;
    for (int b = 0; b < grid; ++b) {
        if (partial[3 * b]) return fail(result, SpMVError::INVALID_FORMAT);
        diff |= static_cast<unsigned long long>(partial[3 * b + 1]) |
                (static_cast<unsigned long long>(partial[3 * b + 2]) << 32);
    }
    return layout.narrow() ? build_sorted<uint32_t>(C, q, layout, diff, plan, result, s)
                           : build_sorted<uint64_t>(C, q, layout, diff, plan, result, s);
}

} // namespace

} // namespace assemble
} // namespace detail

CooResult csr_from_coo_gpu(CSRMatrix* C, int num_rows, int num_cols, int n, const int* d_rows, const int* d_cols,
                           const float* d_vals, const CooConfig* config, CooPlan** plan) {
    using namespace detail;
    CooResult result;
    result.tile_entries = assemble::kTileEntries;
    const CooConfig defaults;
    const CooConfig& cfg = config ? *config : defaults;
    result.error_code = assemble::build_check(C, num_rows, num_cols, n, d_rows, d_cols, d_vals, cfg);
    if (result.error_code != 0) return result;
    CooPlan* made = nullptr;
    const assemble::Request q{num_rows, num_cols, n, d_rows, d_cols, d_vals, cfg.duplicates};
    assemble::build(C, q, plan ? &made : nullptr, &result, current_stream());
    if (plan && result.error_code == 0) *plan = made;
    return result;
}

int csr_coo_refill_async(const CooPlan* plan, CSRMatrix* C, const float* d_vals, hipStream_t stream) {
    using namespace detail;
    const int status = assemble::refill_check(plan, C, d_vals);
    if (status != 0) return status;
    csr_invalidate_gpu_cache(C);          // a tiled plan, transpose or schedule built from the old values
    if (plan->nnz_out == 0) return 0;
    assemble::assemble_numeric_kernel<<<dev::vec_grid(plan->nnz_out), dev::kBlock, 0, stream>>>(
        plan->d_order, plan->d_segments, d_vals, plan->nnz_out, C->d_values);
    if (hipGetLastError() != hipSuccess) return code(SpMVError::KERNEL_LAUNCH);
    return 0;
}

int csr_coo_refill(const CooPlan* plan, CSRMatrix* C, const float* d_vals) {
    using namespace detail;
    hipStream_t s = current_stream();
    const int status = csr_coo_refill_async(plan, C, d_vals, s);
    if (status != 0) return status;
    return stream_finished(s);
}

void coo_plan_destroy(CooPlan* plan) {
    if (!plan) return;
    if (plan->d_order) (void)hipFree(plan->d_order);
    if (plan->d_segments) (void)hipFree(plan->d_segments);
    delete plan;
}

int csr_row_indices_gpu(const CSRMatrix* A, int* d_rows) {
    using namespace detail;
    bool nothing = false;
    const int status = assemble::row_indices_check(A, d_rows, &nothing);
    if (status != 0 || nothing) return status;
    hipStream_t s = current_stream();
    const int checked = structure_checked(A, s);
    if (checked != 0) return checked;
    if (A->nnz == 0) return 0;
    const bool ok = launch_expand_rows(A->d_row_ptrs, A->num_rows, A->nnz, d_rows, s) == hipSuccess;
    if (hipStreamSynchronize(s) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}

} // namespace spmv
