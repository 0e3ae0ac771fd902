// transpose.hip — device CSR transpose AT = A^T: validated, stable, deterministic, no atomics.
//
// Row c of AT holds A's entries of column c in ascending source position p: its column index is p's row in A,
// its value A.values[p] bit for bit.  The order is that of a stable sort of the entries by column, done as an
// LSD radix sort with 8-bit digits:
//   validate    one kernel: row_ptrs[0] == 0, non-decreasing, row_ptrs[rows] == nnz, every column in
//               [0, num_cols); per workgroup a flag and the OR of (column ^ column[0]) — digits whose bits never
//               differ are constant and their passes are skipped.  The host reads these before it allocates.
//   expand      the row of every entry (binary search in row_ptrs, narrowed to the workgroup's row range;
//               launch_expand_rows of csr_build.hip)
//   per pass    digit counts per 4096-entry tile, stored digit-major; an exclusive scan of them
//               (device_exclusive_scan of csr_build.hip); a stable
//               scatter of (key, row, value) that ranks inside a wavefront by ballot + mbcnt and across the
//               wavefronts and rounds of a tile through LDS.  The last pass writes AT's arrays directly.
//   row_ptrs    AT.row_ptrs[c] = lower_bound(sorted keys, c): one thread per column, empty columns included.
// Counting is done by wavefront matching as well, so no kernel here uses an atomic of any kind.
#include "internal.h"
#include "device_common.h"

#include <algorithm>
#include <vector>

namespace spmv {
namespace detail {

namespace {

constexpr int kThreads = 256;                 // 4 wavefronts per workgroup
constexpr int kRounds = 16;                   // rounds of 256 entries per tile
constexpr int kTile = kThreads * kRounds;     // 4096 entries per tile
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

// ---- validation: partial[2b] = violation seen by workgroup b, partial[2b+1] = OR of (col ^ col[0]) ----
__global__ __launch_bounds__(kThreads) void transpose_validate_kernel(const int* __restrict__ rp,
                                                                      const int* __restrict__ ci, int rows, int cols,
                                                                      long long nnz, int* __restrict__ partial) {
    __shared__ int s_bad[kThreads / 64];
    __shared__ unsigned s_diff[kThreads / 64];
    const int ref = nnz > 0 ? ci[0] : 0;
    const long long work = std::max(nnz, rp ? static_cast<long long>(rows) + 1 : 0LL);
    bool bad = false;
    unsigned diff = 0;
    for (long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x; i < work;
         i += static_cast<long long>(gridDim.x) * kThreads) {
        if (rp && i <= rows) {
            const int v = rp[i];
            if (i == 0 && v != 0) bad = true;
            if (i == rows && v != nnz) bad = true;
            if (i < rows && v > rp[i + 1]) bad = true;
        }
        if (i < nnz) {
            const int c = ci[i];
            if (c < 0 || c >= cols) bad = true;
            diff |= static_cast<unsigned>(c ^ ref);
        }
    }
    for (int off = 32; off > 0; off >>= 1) diff |= __shfl_xor(diff, off, 64);
    const unsigned long long any_bad = __ballot(bad);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_bad[wave] = any_bad != 0;
        s_diff[wave] = diff;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = 0;
        unsigned d = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            b |= s_bad[w];
            d |= s_diff[w];
        }
        partial[2 * blockIdx.x] = b;
        partial[2 * blockIdx.x + 1] = static_cast<int>(d);
    }
}

// counts[d * num_tiles + t] = entries of tile t whose digit is d
__global__ __launch_bounds__(kThreads) void transpose_count_kernel(const int* __restrict__ keys, long long n,
                                                                   int shift, int num_tiles,
                                                                   int* __restrict__ counts) {
    __shared__ int s_cnt[kThreads / 64][256];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    const long long tile = blockIdx.x * static_cast<long long>(kTile);
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile + r * kThreads + threadIdx.x;
        const bool valid = i < n;
        const unsigned d = valid ? (static_cast<unsigned>(keys[i]) >> shift) & 255u : 0u;
        const unsigned long long m = match_digit(valid, d);
        // the highest lane of each digit group adds the group's size: one writer per (wavefront, digit)
        if (valid && lanes_below(m) == static_cast<unsigned>(__popcll(m)) - 1) s_cnt[wave][d] += __popcll(m);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) total += s_cnt[w][threadIdx.x];
    counts[static_cast<long long>(threadIdx.x) * num_tiles + blockIdx.x] = total;
}

// Stable scatter of one pass.  offsets[d * num_tiles + t] = where tile t's first digit-d entry goes.  A tile is
// walked in rounds of 256 consecutive entries; inside a round entry order is (wavefront, lane) order, so ranks are
// lanes_below() of the wavefront's match mask plus the counts of earlier wavefronts and rounds of the same digit.
__global__ __launch_bounds__(kThreads) void transpose_scatter_kernel(
        const int* __restrict__ keys_in, const int* __restrict__ rows_in, const unsigned* __restrict__ vals_in,
        long long n, int shift, int num_tiles, const int* __restrict__ offsets,
        int* __restrict__ keys_out, int* __restrict__ rows_out, unsigned* __restrict__ vals_out) {
    __shared__ int s_cnt[kThreads / 64][256];     // this round: entries per (wavefront, digit)
    __shared__ int s_base[kThreads / 64][256];    // this round: first output position per (wavefront, digit)
    __shared__ int s_run[256];                    // next output position per digit
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s_cnt[w][threadIdx.x] = 0;
    s_run[threadIdx.x] = offsets[static_cast<long long>(threadIdx.x) * num_tiles + blockIdx.x];
    __syncthreads();
    const long long tile = blockIdx.x * static_cast<long long>(kTile);
    for (int r = 0; r < kRounds; ++r) {
        const long long i = tile + r * kThreads + threadIdx.x;
        const bool valid = i < n;
        int key = 0, row = 0;
        unsigned val = 0;
        if (valid) {
            key = keys_in[i];
            row = rows_in[i];
            val = vals_in[i];
        }
        const unsigned d = (static_cast<unsigned>(key) >> shift) & 255u;
        const unsigned long long m = match_digit(valid, d);
        const int rank = static_cast<int>(lanes_below(m));
        if (valid && rank == __popcll(m) - 1) s_cnt[wave][d] = rank + 1;
        __syncthreads();
        int run = s_run[threadIdx.x];
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            s_base[w][threadIdx.x] = run;
            run += s_cnt[w][threadIdx.x];
            s_cnt[w][threadIdx.x] = 0;
        }
        s_run[threadIdx.x] = run;
        __syncthreads();
        if (valid) {
            const int pos = s_base[wave][d] + rank;
            keys_out[pos] = key;
            rows_out[pos] = row;
            vals_out[pos] = val;
        }
    }
}

// AT.row_ptrs[c] = number of sorted keys < c, for c in [0, cols]
__global__ __launch_bounds__(kThreads) void transpose_row_ptrs_kernel(const int* __restrict__ keys, long long n,
                                                                      int cols, int* __restrict__ at_rp) {
    const long long c = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (c > cols) return;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    at_rp[c] = static_cast<int>(lo);
}

unsigned blocks_for(long long n, long long per) { return static_cast<unsigned>((n + per - 1) / per); }

// the build's scratch, freed when it goes out of scope (after the build has completed)
struct Scratch {
    std::vector<void*> held;
    template <typename T>
    bool get(T** p, size_t count) {
        *p = nullptr;
        if (count == 0) return true;
        if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            return false;
        }
        held.push_back(*p);
        return true;
    }
    ~Scratch() {
        for (void* p : held) (void)hipFree(p);
    }
};

} // namespace

int transpose_build(const CSRMatrix* A, DeviceCsrArrays* out, hipStream_t s) {
    *out = DeviceCsrArrays();
    if (!A) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    const int rows = A->num_rows, cols = A->num_cols;
    const long long nnz = A->nnz;

    // ---- validation: one kernel, one read of its per-workgroup flags, before anything is allocated ----
    unsigned diff = 0;
    const int* rp = A->d_row_ptrs;
    if (rp || nnz > 0) {
        const long long work = std::max(nnz, rp ? static_cast<long long>(rows) + 1 : 0LL);
        const unsigned grid = std::min<unsigned>(kValidateGrid, std::max(1u, blocks_for(work, kThreads)));
        int* d_flags = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&d_flags), 2 * sizeof(int) * grid) != hipSuccess) {
            (void)hipGetLastError();
            return code(SpMVError::CUDA_MALLOC);
        }
        std::vector<int> flags(2 * grid);
        transpose_validate_kernel<<<grid, kThreads, 0, s>>>(rp, A->d_col_indices, rows, cols, nnz, d_flags);
        const bool ok = hipGetLastError() == hipSuccess &&
                        hipMemcpyAsync(flags.data(), d_flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost,
                                       s) == hipSuccess &&
                        hipStreamSynchronize(s) == hipSuccess;
        (void)hipFree(d_flags);
        if (!ok) return code(SpMVError::KERNEL_LAUNCH);
        for (unsigned b = 0; b < grid; ++b) {
            if (flags[2 * b]) return code(SpMVError::INVALID_FORMAT);
            diff |= static_cast<unsigned>(flags[2 * b + 1]);
        }
    }

    // ---- AT's arrays ----
    DeviceCsrArrays at;
    if (at.alloc(static_cast<long long>(cols) + 1, nnz) != hipSuccess) return code(SpMVError::CUDA_MALLOC);

    // passes: the digits (of four) in which some column differs from column[0]
    std::vector<int> shifts;
    for (int d = 0; d < 4; ++d) {
        if ((diff >> (8 * d)) & 255u) shifts.push_back(8 * d);
    }
    const int passes = static_cast<int>(shifts.size());
    const int* sorted_keys = A->d_col_indices;            // no pass: every column is equal (or there are none)
    bool launched = true;
    {
        Scratch scratch;
        const long long tiles = (nnz + kTile - 1) / kTile;
        const std::vector<long long> levels = device_scan_levels(256 * tiles);
        int *keys_a = nullptr, *keys_b = nullptr, *rows_b = nullptr, *counts = nullptr;
        unsigned* vals_b = nullptr;
        const bool got = passes == 0 ||
            (scratch.get(&keys_a, nnz) && scratch.get(&rows_b, nnz) &&
             (passes < 2 || (scratch.get(&keys_b, nnz) && scratch.get(&vals_b, nnz))) &&
             scratch.get(&counts, 256 * tiles + device_scan_sums(levels)));
        if (!got) {
            at.release();
            return code(SpMVError::CUDA_MALLOC);
        }
        if (nnz > 0) {
            // pass j writes set A = (keys_a, AT.col_indices, AT.values) when passes - j is even, set B otherwise;
            // the first pass reads the expanded rows from the set it does not write
            int* row_of = passes % 2 == 1 ? rows_b : at.col_indices;
            launched = launched && launch_expand_rows(rp, rows, nnz, row_of, s) == hipSuccess;
            if (passes == 0) {
                launched = launched && hipMemcpyAsync(at.values, A->d_values, nnz * sizeof(float),
                                                      hipMemcpyDeviceToDevice, s) == hipSuccess;
            }
            const int* k_in = A->d_col_indices;
            const int* r_in = row_of;
            const unsigned* v_in = reinterpret_cast<const unsigned*>(A->d_values);
            for (int j = 1; j <= passes && launched; ++j) {
                const bool to_a = (passes - j) % 2 == 0;
                int* k_out = to_a ? keys_a : keys_b;
                int* r_out = to_a ? at.col_indices : rows_b;
                unsigned* v_out = to_a ? reinterpret_cast<unsigned*>(at.values) : vals_b;
                const int shift = shifts[j - 1];
                transpose_count_kernel<<<static_cast<unsigned>(tiles), kThreads, 0, s>>>(
                    k_in, nnz, shift, static_cast<int>(tiles), counts);
                launched = hipGetLastError() == hipSuccess &&
                           device_exclusive_scan(counts, levels, counts + levels[0], s) == hipSuccess;
                transpose_scatter_kernel<<<static_cast<unsigned>(tiles), kThreads, 0, s>>>(
                    k_in, r_in, v_in, nnz, shift, static_cast<int>(tiles), counts, k_out, r_out, v_out);
                launched = launched && hipGetLastError() == hipSuccess;
                k_in = k_out;
                r_in = r_out;
                v_in = v_out;
            }
            if (passes > 0) sorted_keys = keys_a;
        }
        if (launched) {
            transpose_row_ptrs_kernel<<<blocks_for(static_cast<long long>(cols) + 1, kThreads), kThreads, 0, s>>>(
                sorted_keys, nnz, cols, at.row_ptrs);
            launched = hipGetLastError() == hipSuccess;
        }
        launched = hipStreamSynchronize(s) == hipSuccess && launched;
    }   // (scratch freed here)
    if (!launched) {
        at.release();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    *out = at;
    return code(SpMVError::SUCCESS);
}

} // namespace detail
} // namespace spmv
