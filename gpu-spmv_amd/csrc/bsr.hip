// bsr.hip — block CSR on the device (include/spmv/bsr.h): CSR -> BSR with its values-only refill and
// the counting pass alone, BSR -> CSR, and y = A x on a BSRMatrix.  Everything is templated on the block size B; no
// sort, no float atomics, no LDS, no workgroup waits for another.
//
// CSR -> BSR.  A group of LANES lanes owns a block row and strides over the entries of its B rows, which are one
// contiguous range of A, in tiles of LANES.
//   COUNT    an entry OWNS its block when it is the first of its row with that block column and no earlier row of the
//            block row holds a column of the block (a binary search per earlier row).  The group counts its owners
//            (a __ballot per tile) and leaves for every entry the number of owners before it in the block row, with
//            the owner flag in the sign.  It also checks that every column is above its left neighbour.  An exclusive
//            scan turns the counts into the block row pointers.
//   COLUMNS  the rank of block column J in its block row is the number of owners with a smaller block column: for
//            each of the B rows, the owners left of the row's lower bound of column J*B, read from the prefixes.  Every
//            owner writes J at its rank.
//   SCATTER  every entry finds its block by a search in the finished block row and writes its value into the zeroed
//            value array: one writer per slot.  The same kernel is bsr_from_csr_numeric: it trusts nothing (row
//            pointers, columns and B's block row are checked before they are followed) and flags an entry without
//            a block.
// Neither ranks nor slots depend on LANES.
//
// y = A x.  bsr_rows_kernel: one lane per scalar row, spmv_cpu_bsr's order, multiply and add rounded separately.
// bsr_lanes_kernel: a group of LANES lanes per block row, a lane takes whole blocks (16-byte loads where B*B is a
// multiple of four and the value array is 16-byte aligned; B = 3 and misaligned views take dword loads), holds B
// accumulators, and group_sum folds each of them.  At B*B flops per 4 B of index the kernel stays far below the
// machine balance, so no MFMA (the argument at the head of kernels.hip).
#include "bsr_device.h"
#include "bsr_impl.h"
#include "device_common.h"
#include "internal.h"

#include <algorithm>
#include <climits>
#include <cstdint>
#include <type_traits>
#include <vector>

namespace spmv {
namespace detail {
namespace bsr {

namespace {

using dev::capped_grid;
using dev::f32x4;
using dev::group_sum;
using dev::kBlock;

constexpr int kWaves = kBlock / 64;

// the bits of this lane's group in a wavefront ballot
template <int LANES>
__device__ __forceinline__ unsigned long long group_bits(unsigned long long ballot) {
    if constexpr (LANES == 64) {
        return ballot;
    } else {
        return (ballot >> ((threadIdx.x & 63) / LANES * LANES)) & ((1ull << LANES) - 1ull);
    }
}

// first p in [lo, hi) with cols[p] >= want, hi when there is none; never reads outside [lo, hi)
__device__ __forceinline__ int lower_bound(const int* __restrict__ cols, int lo, int hi, int want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cols[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

enum Mode { COUNT = 0, COLUMNS = 1 };

struct ConvArgs {
    const int* rp;            // A
    const int* ci;
    const float* va;
    int m, n;
    long long nnz;
    int block_rows;
    int* counts;              // COUNT: [block_rows + 1], counts[block_rows] = 0
    int* owners;              // COUNT writes, COLUMNS reads: [nnz] owners before the entry in its block row, ~that for
                              // an entry that owns nothing; null for the counting pass alone
    long long* partial;       // COUNT: per wavefront of the grid {blocks, positions inside the matrix, most blocks in a block row}
    int* flag;                // COUNT: a column not above its left neighbour; SCATTER: any check failed
    const int* brp;           // COLUMNS, SCATTER: B
    int* bc;
    float* bv;
    int num_blocks;
};

// The row pointers of block row I: v[k] = rp[min(I*B + k, m)], so rows past the matrix are empty ranges.
template <int B>
__device__ __forceinline__ void load_block_row(const int* __restrict__ rp, long long I, int m, int (&v)[B + 1]) {
    const long long r0 = I * B;
#pragma unroll
    for (int k = 0; k <= B; ++k) v[k] = rp[min(r0 + k, static_cast<long long>(m))];
}

// the row of the block row that holds entry p: r, and its range [begin, end) (constant indices only: no scratch)
template <int B>
__device__ __forceinline__ void row_of_entry(const int (&v)[B + 1], int p, int* r, int* begin, int* end) {
    *r = 0;
    *begin = v[0];
    *end = v[1];
#pragma unroll
    for (int k = 1; k < B; ++k) {
        if (v[k] <= p) {
            *r = k;
            *begin = v[k];
            *end = v[k + 1];
        }
    }
}

// COUNT and COLUMNS over a matrix whose row pointers and column range structure_checked has accepted.
template <int B, int LANES, int MODE>
__global__ __launch_bounds__(kBlock) void bsr_symbolic_kernel(ConvArgs g) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    const unsigned long long below = (1ull << lane) - 1ull;
    bool bad = false;
    long long sum_blocks = 0, sum_positions = 0, top = 0;
    if (MODE == COUNT && blockIdx.x == 0 && threadIdx.x == 0) g.counts[g.block_rows] = 0;

    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < g.block_rows;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long I = first + slot;
        int v[B + 1];
#pragma unroll
        for (int k = 0; k <= B; ++k) v[k] = 0;
        if (I < g.block_rows) load_block_row<B>(g.rp, I, g.m, v);
        const int lo = v[0], hi = v[B];
        const int rows_here = static_cast<int>(min(static_cast<long long>(B), g.m - I * B));
        const int total = MODE == COLUMNS && I < g.block_rows ? g.brp[I + 1] - g.brp[I] : 0;
        int carry = 0;
        for (int t0 = lo; t0 < hi; t0 += LANES) {
            const int p = t0 + lane;
            const bool active = p < hi;
            if (MODE == COUNT) {
                bool owner = false;
                int J = 0;
                if (active) {
                    int r, begin, end;
                    row_of_entry<B>(v, p, &r, &begin, &end);
                    const int col = g.ci[p];
                    J = col / B;
                    owner = true;
                    if (p > begin) {
                        const int left = g.ci[p - 1];
                        if (left >= col) bad = true;
                        owner = left / B != J;
                    }
#pragma unroll
                    for (int k = 0; k < B - 1; ++k) {
                        if (owner && k < r) {
                            const int q = lower_bound(g.ci, v[k], v[k + 1], J * B);
                            if (q < v[k + 1] && g.ci[q] / B == J) owner = false;
                        }
                    }
                }
                const unsigned long long bits = group_bits<LANES>(__ballot(owner));
                if (active && g.owners) {
                    const int before = carry + __popcll(bits & below);
                    g.owners[p] = owner ? before : ~before;
                }
                if (owner) sum_positions += static_cast<long long>(rows_here) * min(B, g.n - J * B);
                carry += __popcll(bits);
            } else if (active) {
                const int mine = g.owners[p];
                if (mine >= 0) {
                    const int J = g.ci[p] / B;
                    int rank = 0;
#pragma unroll
                    for (int k = 0; k < B; ++k) {
                        const int q = lower_bound(g.ci, v[k], v[k + 1], J * B);
                        int left = total, start = total;             // owners before an index: the prefix, or all of them at hi
                        if (q < hi) {
                            left = g.owners[q];
                            left = left >= 0 ? left : ~left;
                        }
                        if (v[k] < hi) {
                            start = g.owners[v[k]];
                            start = start >= 0 ? start : ~start;
                        }
                        rank += left - start;
                    }
                    g.bc[g.brp[I] + rank] = J;
                }
            }
        }
        if (MODE == COUNT && I < g.block_rows && lane == 0) {
            g.counts[I] = carry;
            sum_blocks += carry;
            top = max(top, static_cast<long long>(carry));
        }
    }

    if (MODE == COUNT) {
        for (int off = 32; off > 0; off >>= 1) {
            sum_blocks += __shfl_xor(sum_blocks, off, 64);
            sum_positions += __shfl_xor(sum_positions, off, 64);
            top = max(top, __shfl_xor(top, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            long long* mine = g.partial + 3 * (static_cast<long long>(blockIdx.x) * kWaves + (threadIdx.x >> 6));
            mine[0] = sum_blocks;
            mine[1] = sum_positions;
            mine[2] = top;
        }
        if (__any(bad) && (threadIdx.x & 63) == 0) *g.flag = 1;     // (every writer stores the same 1)
    }
}

// SCATTER: the values of A into B's zeroed value array.  Nothing is trusted: a block row whose row pointers are not
// 0 <= begin <= end <= nnz in order (with rp[0] == 0 and rp[m] == nnz), whose range in B is not inside
// [0, num_blocks], a column outside [0, n) and an entry whose block B does not hold all raise the flag, and nothing
// of them is followed.
template <int B, int LANES>
__global__ __launch_bounds__(kBlock) void bsr_scatter_kernel(ConvArgs g) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    bool bad = false;
    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < g.block_rows;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long I = first + slot;
        if (I >= g.block_rows) continue;
        int v[B + 1];
        load_block_row<B>(g.rp, I, g.m, v);
        bool ok = v[0] >= 0 && v[B] <= g.nnz;
#pragma unroll
        for (int k = 0; k < B; ++k) ok = ok && v[k] <= v[k + 1];
        if (I == 0 && v[0] != 0) ok = false;
        if (I == g.block_rows - 1 && v[B] != g.nnz) ok = false;
        const int b0 = g.brp[I], b1 = g.brp[I + 1];
        if (b0 < 0 || b0 > b1 || b1 > g.num_blocks) ok = false;
        if (!ok) {
            bad = true;
            continue;
        }
        for (int p = v[0] + lane; p < v[B]; p += LANES) {
            int r, begin, end;
            row_of_entry<B>(v, p, &r, &begin, &end);
            const int col = g.ci[p];
            if (col < 0 || col >= g.n) {
                bad = true;
                continue;
            }
            const int J = col / B;
            const int at = dev::find_column(g.bc, b0, b1, J);
            if (at < 0) {
                bad = true;
                continue;
            }
            g.bv[(static_cast<long long>(at) * B + r) * B + (col - J * B)] = g.va[p];
        }
    }
    if (bad) *g.flag = 1;
}

// ---- BSR -> CSR ------------------------------------------------------------------------------------------------
// block columns strictly ascending inside every block row (row pointers and the column range are checked already)
__global__ __launch_bounds__(kBlock) void bsr_ascending_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                                               int block_rows, int* flag) {
    bool bad = false;
    for (long long I = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; I < block_rows;
         I += static_cast<long long>(gridDim.x) * kBlock) {
        for (int p = brp[I] + 1; p < brp[I + 1]; ++p) bad = bad || bc[p] <= bc[p - 1];
    }
    if (bad) *flag = 1;
}

__device__ __forceinline__ bool keeps(float v, int keep_zeros) {
    return keep_zeros || (__float_as_uint(v) & 0x7FFFFFFFu) != 0;
}

// counts[i] = entries of scalar row i (counts[m] = 0); *total += all of them
__global__ __launch_bounds__(kBlock) void bsr_to_csr_count_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                                                  const float* __restrict__ bv, int m, int n, int b,
                                                                  int keep_zeros, int* counts,
                                                                  unsigned long long* total) {
    long long sum = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[m] = 0;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < m;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int I = static_cast<int>(i / b), r = static_cast<int>(i % b);
        long long count = 0;
        for (int p = brp[I]; p < brp[I + 1]; ++p) {
            const int width = min(b, n - bc[p] * b);
            const float* line = bv + (static_cast<long long>(p) * b + r) * b;
            for (int c = 0; c < width; ++c) count += keeps(line[c], keep_zeros) ? 1 : 0;
        }
        counts[i] = count > INT_MAX ? INT_MAX : static_cast<int>(count);
        sum += count;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, static_cast<unsigned long long>(sum));
}

__global__ __launch_bounds__(kBlock) void bsr_to_csr_fill_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                                                 const float* __restrict__ bv, int m, int n, int b,
                                                                 int keep_zeros, const int* __restrict__ rp,
                                                                 int* __restrict__ ci, float* __restrict__ va) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < m;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int I = static_cast<int>(i / b), r = static_cast<int>(i % b);
        int out = rp[i];
        for (int p = brp[I]; p < brp[I + 1]; ++p) {
            const int first = bc[p] * b;
            const int width = min(b, n - first);
            const float* line = bv + (static_cast<long long>(p) * b + r) * b;
            for (int c = 0; c < width; ++c) {
                const float v = line[c];
                if (keeps(v, keep_zeros)) {
                    ci[out] = first + c;
                    va[out] = v;
                    ++out;
                }
            }
        }
    }
}

// ---- y = A x ---------------------------------------------------------------------------------------------------
// spmv_cpu_bsr's sum: one lane per scalar row, blocks in stored order, every product and every sum rounded
template <int B>
__global__ __launch_bounds__(kBlock) void bsr_rows_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                                          const float* __restrict__ bv, const float* __restrict__ x,
                                                          float* __restrict__ y, int m, int n) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < m;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int I = static_cast<int>(i / B), r = static_cast<int>(i % B);
        float s = 0.0f;
        for (int p = brp[I]; p < brp[I + 1]; ++p) {
            const int first = bc[p] * B;
            const float* line = bv + (static_cast<long long>(p) * B + r) * B;
#pragma unroll
            for (int c = 0; c < B; ++c) {
                if (first + c < n) s = __fadd_rn(s, __fmul_rn(line[c], x[first + c]));
            }
        }
        y[i] = s;
    }
}

// A group of LANES lanes per block row (for_each_block_row_dot, bsr_device.h).
template <int B, int LANES, bool WIDE>
__global__ __launch_bounds__(kBlock) void bsr_lanes_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                                           const float* __restrict__ bv, const float* __restrict__ x,
                                                           float* __restrict__ y, int m, int n, int block_rows) {
    for_each_block_row_dot<B, LANES, WIDE>(brp, bc, bv, x, m, n, block_rows,
                                           [&](long long row, float sum) { y[row] = sum; });
}

// ---- host side -------------------------------------------------------------------------------------------------

template <int MODE>
hipError_t launch_symbolic(int block_dim, int lanes, int grid, const ConvArgs& args, hipStream_t s) {
    return with_block_dim(block_dim, [&](auto Bc) {
        return dev::with_lanes(lanes, [&](auto L) {
            bsr_symbolic_kernel<decltype(Bc)::value, decltype(L)::value, MODE><<<grid, kBlock, 0, s>>>(args);
            return hipGetLastError();
        });
    });
}

hipError_t launch_scatter(int block_dim, int lanes, int grid, const ConvArgs& args, hipStream_t s) {
    return with_block_dim(block_dim, [&](auto Bc) {
        return dev::with_lanes(lanes, [&](auto L) {
            bsr_scatter_kernel<decltype(Bc)::value, decltype(L)::value><<<grid, kBlock, 0, s>>>(args);
            return hipGetLastError();
        });
    });
}

ConvArgs args_of(const CSRMatrix* A, int block_dim) {
    ConvArgs args{};
    args.rp = A->d_row_ptrs;
    args.ci = A->d_col_indices;
    args.va = A->d_values;
    args.m = A->num_rows;
    args.n = A->num_cols;
    args.nnz = A->nnz;
    args.block_rows = blocks_along(A->num_rows, block_dim);
    return args;
}

// What the counting pass and the scan leave: the block row pointers, the owner prefixes and the totals.
struct Counted {
    DevBuf<int> counts;       // [block_rows + 1], scanned
    DevBuf<int> owners;       // [nnz], when asked for
    long long blocks = 0, positions = 0, top = 0;
    int lanes = 0, launches = 0;
};

// Check 4 and the counting pass on `s`, waited for; ev (may be null) gets events 0 and 1 around the pass and the scan.
int count_pass(const CSRMatrix* A, int block_dim, bool keep_owners, Counted* out, Events* ev, hipStream_t s) {
    ConvArgs args = args_of(A, block_dim);
    out->lanes = lanes_for(A->nnz, args.block_rows);
    if (dev_alloc(&out->counts, static_cast<long long>(args.block_rows) + 1) != hipSuccess) return fail(SpMVError::CUDA_MALLOC);
    if (A->num_rows == 0 || A->nnz == 0) {          // no blocks: the row pointers are all zero
        if (A->num_rows > 0) {
            const int checked = structure_checked(A, s);
            if (checked != 0) return checked;
        }
        if (hipMemsetAsync(out->counts.get(), 0, (static_cast<size_t>(args.block_rows) + 1) * sizeof(int), s) != hipSuccess) {
            return fail(SpMVError::KERNEL_LAUNCH);
        }
        return stream_finished(s);
    }
    const int checked = structure_checked(A, s);    // row pointers and the column range, before anything follows them
    if (checked != 0) return checked;

    const int grid = capped_grid(args.block_rows, kBlock / out->lanes);
    const std::vector<long long> levels = device_scan_levels(static_cast<long long>(args.block_rows) + 1);
    const size_t waves = static_cast<size_t>(grid) * kWaves;
    DevBuf<int> scan_sums, flag;
    DevBuf<long long> partial;
    if (dev_alloc(&scan_sums, device_scan_sums(levels)) != hipSuccess || dev_alloc(&flag, 1) != hipSuccess ||
        dev_alloc(&partial, 3LL * static_cast<long long>(waves)) != hipSuccess ||
        (keep_owners && dev_alloc(&out->owners, A->nnz) != hipSuccess)) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    args.counts = out->counts.get();
    args.owners = keep_owners ? out->owners.get() : nullptr;
    args.partial = partial.get();
    args.flag = flag.get();
    std::vector<long long> host_partial(3 * waves);
    int bad = 0;
    bool ok = hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
              (!ev || hipEventRecord(ev->e[0], s) == hipSuccess) &&
              launch_symbolic<COUNT>(block_dim, out->lanes, grid, args, s) == hipSuccess &&
              device_exclusive_scan(out->counts.get(), levels, scan_sums.get(), s) == hipSuccess &&
              (!ev || hipEventRecord(ev->e[1], s) == hipSuccess) &&
              hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess &&
              hipMemcpyAsync(host_partial.data(), partial.get(), host_partial.size() * sizeof(long long),
                             hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok) return fail(SpMVError::KERNEL_LAUNCH);
    out->launches = 2 + device_scan_launches(levels);       // the structure check, the counting pass, the scan
    if (bad) return fail(SpMVError::INVALID_FORMAT);
    for (size_t w = 0; w < waves; ++w) {
        out->blocks += host_partial[3 * w];
        out->positions += host_partial[3 * w + 1];
        out->top = std::max(out->top, host_partial[3 * w + 2]);
    }
    return 0;
}

int build(BSRMatrix* B, const CSRMatrix* A, int block_dim, BsrBuildResult* result, hipStream_t s) {
    *result = BsrBuildResult();
    const int status = from_csr_check(B, A, block_dim);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    const TraceRange range("spmv:bsr_from_csr_gpu");
    Events ev;
    if (!ev.ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    Counted counted;
    const int done = count_pass(A, block_dim, true, &counted, &ev, s);
    result->lanes = counted.lanes;
    result->launches = counted.launches;
    if (done != 0) return fail(result, static_cast<SpMVError>(done));
    if (counted.blocks > INT_MAX) return fail(result, SpMVError::INVALID_DIMENSION);
    const int num_blocks = static_cast<int>(counted.blocks);

    DevBuf<int> block_cols;
    DevBuf<float> values;
    if (num_blocks > 0) {
        (void)hipEventElapsedTime(&result->symbolic_ms, ev.e[0], ev.e[1]);
        const size_t value_bytes = static_cast<size_t>(num_blocks) * block_dim * block_dim * sizeof(float);
        if (dev_alloc(&block_cols, num_blocks) != hipSuccess ||
            dev_alloc(&values, static_cast<long long>(value_bytes / sizeof(float))) != hipSuccess) {
            return fail(result, SpMVError::CUDA_MALLOC);
        }
        ConvArgs args = args_of(A, block_dim);
        DevBuf<int> flag;
        if (dev_alloc(&flag, 1) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
        args.owners = counted.owners.get();
        args.flag = flag.get();
        args.brp = counted.counts.get();
        args.bc = block_cols.get();
        args.bv = values.get();
        args.num_blocks = num_blocks;
        const int grid = capped_grid(args.block_rows, kBlock / counted.lanes);
        int bad = 0;
        bool ok = hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
                  hipEventRecord(ev.e[2], s) == hipSuccess &&
                  launch_symbolic<COLUMNS>(block_dim, counted.lanes, grid, args, s) == hipSuccess &&
                  hipMemsetAsync(values.get(), 0, value_bytes, s) == hipSuccess &&
                  launch_scatter(block_dim, counted.lanes, grid, args, s) == hipSuccess &&
                  hipEventRecord(ev.e[3], s) == hipSuccess &&
                  hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        if (!ok || bad) return fail(result, SpMVError::KERNEL_LAUNCH);     // (the scatter cannot miss a block it counted)
        (void)hipEventElapsedTime(&result->numeric_ms, ev.e[2], ev.e[3]);
        result->launches += 2;
    }
    adopt_device(B, A->num_rows, A->num_cols, block_dim, num_blocks, counted.counts.release(), block_cols.release(),
                 values.release());
    result->num_blocks = num_blocks;
    result->max_block_row = static_cast<int>(counted.top);
    result->fill = counted.positions > 0
                       ? static_cast<float>(static_cast<double>(A->nnz) / static_cast<double>(counted.positions)) : 0.0f;
    return 0;
}

int refill(BSRMatrix* B, const CSRMatrix* A, BsrBuildResult* result, hipStream_t s) {
    *result = BsrBuildResult();
    const int status = numeric_check(B, A);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    const TraceRange range("spmv:bsr_from_csr_numeric");
    ConvArgs args = args_of(A, B->block_dim);
    const int lanes = lanes_for(A->nnz, args.block_rows);
    result->lanes = lanes;
    result->num_blocks = B->num_blocks;
    if (A->num_rows == 0) return 0;                  // (no rows: no entries, by check 3, and B holds no values)

    DevBuf<int> flag;
    if (dev_alloc(&flag, 1) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    args.flag = flag.get();
    args.brp = B->d_block_row_ptrs;
    args.bc = B->d_block_cols;
    args.bv = B->d_values;
    args.num_blocks = B->num_blocks;
    const size_t value_bytes = static_cast<size_t>(B->num_blocks) * B->block_dim * B->block_dim * sizeof(float);
    EventPair& ev = thread_events();
    int bad = 0;
    bool ok = ev.start && ev.stop && hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
              hipEventRecord(ev.start, s) == hipSuccess &&
              (value_bytes == 0 || hipMemsetAsync(B->d_values, 0, value_bytes, s) == hipSuccess) &&
              launch_scatter(B->block_dim, lanes, capped_grid(args.block_rows, kBlock / lanes), args, s) == hipSuccess &&
              hipEventRecord(ev.stop, s) == hipSuccess &&
              hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    result->launches = 1;
    if (bad) return fail(result, SpMVError::INVALID_FORMAT);
    (void)hipEventElapsedTime(&result->numeric_ms, ev.start, ev.stop);
    bsr_invalidate_gpu_cache(B);
    return 0;
}

int to_csr(CSRMatrix* A, const BSRMatrix* B, int keep_zeros, hipStream_t s) {
    const int status = to_csr_check(A, B);
    if (status != 0) return status;
    const TraceRange range("spmv:bsr_to_csr_gpu");
    const int m = B->num_rows, n = B->num_cols;
    DevBuf<int> counts, flag, scan_sums;
    DevBuf<unsigned long long> total;
    const std::vector<long long> levels = device_scan_levels(static_cast<long long>(m) + 1);
    unsigned long long nnz = 0;
    if (m > 0) {
        // B's block structure is a CSR structure of its own: the row-pointer rule and the column range by the shared check
        CSRMatrix blocks{};
        blocks.num_rows = B->num_block_rows;
        blocks.num_cols = B->num_block_cols;
        blocks.nnz = B->num_blocks;
        blocks.d_row_ptrs = B->d_block_row_ptrs;
        blocks.d_col_indices = B->d_block_cols;
        const int checked = structure_checked(&blocks, s);
        if (checked != 0) return checked;
        if (dev_alloc(&flag, 1) != hipSuccess || dev_alloc(&counts, static_cast<long long>(m) + 1) != hipSuccess ||
            dev_alloc(&scan_sums, device_scan_sums(levels)) != hipSuccess || dev_alloc(&total, 1) != hipSuccess) {
            return fail(SpMVError::CUDA_MALLOC);
        }
        int bad = 0;
        bool ok = hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
                  hipMemsetAsync(total.get(), 0, sizeof(unsigned long long), s) == hipSuccess;
        if (ok) {
            bsr_ascending_kernel<<<dev::vec_grid(B->num_block_rows), kBlock, 0, s>>>(B->d_block_row_ptrs, B->d_block_cols,
                                                                                     B->num_block_rows, flag.get());
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
        }
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        if (!ok) return fail(SpMVError::KERNEL_LAUNCH);
        if (bad) return fail(SpMVError::INVALID_FORMAT);
        bsr_to_csr_count_kernel<<<dev::vec_grid(m), kBlock, 0, s>>>(B->d_block_row_ptrs, B->d_block_cols, B->d_values, m, n,
                                                                    B->block_dim, keep_zeros, counts.get(), total.get());
        ok = hipGetLastError() == hipSuccess &&
             device_exclusive_scan(counts.get(), levels, scan_sums.get(), s) == hipSuccess &&
             hipMemcpyAsync(&nnz, total.get(), sizeof(nnz), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        if (!ok) return fail(SpMVError::KERNEL_LAUNCH);
        if (nnz > static_cast<unsigned long long>(INT_MAX)) return fail(SpMVError::INVALID_DIMENSION);
    } else {
        if (dev_alloc(&counts, 1) != hipSuccess) return fail(SpMVError::CUDA_MALLOC);
        if (hipMemsetAsync(counts.get(), 0, sizeof(int), s) != hipSuccess || stream_finished(s) != 0) {
            return fail(SpMVError::KERNEL_LAUNCH);
        }
    }
    DeviceCsrArrays c;
    const ReleaseOnExit release_c{&c};
    if (c.alloc_entries(static_cast<long long>(nnz)) != hipSuccess) return fail(SpMVError::CUDA_MALLOC);
    if (nnz > 0) {
        bsr_to_csr_fill_kernel<<<dev::vec_grid(m), kBlock, 0, s>>>(B->d_block_row_ptrs, B->d_block_cols, B->d_values, m, n,
                                                                   B->block_dim, keep_zeros, counts.get(), c.col_indices,
                                                                   c.values);
        const int done = stream_finished(s);
        if (done != 0) return done;
    }
    c.row_ptrs = counts.release();
    csr_adopt_device(A, m, n, static_cast<int>(nnz), &c);
    return 0;
}

// ---- SpMV launchers ----
hipError_t launch_rows(const BSRMatrix* A, const float* d_x, float* d_y, hipStream_t s) {
    return with_block_dim(A->block_dim, [&](auto Bc) {
        bsr_rows_kernel<decltype(Bc)::value><<<capped_grid(A->num_rows, kBlock), kBlock, 0, s>>>(
            A->d_block_row_ptrs, A->d_block_cols, A->d_values, d_x, d_y, A->num_rows, A->num_cols);
        return hipGetLastError();
    });
}

hipError_t launch_lanes(const BSRMatrix* A, const float* d_x, float* d_y, int lanes, hipStream_t s) {
    const int grid = capped_grid(A->num_block_rows, kBlock / lanes);
    const bool wide = aligned16(A->d_values);
    return with_block_dim(A->block_dim, [&](auto Bc) {
        constexpr int B = decltype(Bc)::value;
        return dev::with_lanes(lanes, [&](auto L) {
            constexpr int LANES = decltype(L)::value;
            if (B * B % 4 == 0 && wide) {
                bsr_lanes_kernel<B, LANES, B * B % 4 == 0><<<grid, kBlock, 0, s>>>(
                    A->d_block_row_ptrs, A->d_block_cols, A->d_values, d_x, d_y, A->num_rows, A->num_cols, A->num_block_rows);
            } else {
                bsr_lanes_kernel<B, LANES, false><<<grid, kBlock, 0, s>>>(
                    A->d_block_row_ptrs, A->d_block_cols, A->d_values, d_x, d_y, A->num_rows, A->num_cols, A->num_block_rows);
            }
            return hipGetLastError();
        });
    });
}

bool block_size_ok(const SpMVConfig* config) { return config->block_size > 0 && config->block_size <= 1024; }

hipError_t enqueue(const BSRMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config, hipStream_t s) {
    if (A->num_blocks == 0) return launch_fill_zero(d_y, A->num_rows, s);
    if (config->kernel_type == SpMVConfig::VECTOR_CSR || config->kernel_type == SpMVConfig::MERGE_PATH) {
        return launch_lanes(A, d_x, d_y, product_lanes(A), s);
    }
    return launch_rows(A, d_x, d_y, s);
}

} // namespace

} // namespace bsr
} // namespace detail

int bsr_from_csr_gpu(BSRMatrix* B, const CSRMatrix* A, int block_dim, BsrBuildResult* result) {
    BsrBuildResult local;
    return detail::bsr::build(B, A, block_dim, result ? result : &local, detail::current_stream());
}

int bsr_from_csr_numeric(BSRMatrix* B, const CSRMatrix* A, BsrBuildResult* result) {
    BsrBuildResult local;
    return detail::bsr::refill(B, A, result ? result : &local, detail::current_stream());
}

int csr_block_count_gpu(const CSRMatrix* A, int block_dim, long long* blocks) {
    using namespace detail;
    if (!blocks) return code(SpMVError::INVALID_ARGUMENT);
    BSRMatrix none{};
    const int status = bsr::from_csr_check(&none, A, block_dim);
    if (status != 0) return status;
    bsr::Counted counted;
    const int done = bsr::count_pass(A, block_dim, false, &counted, nullptr, current_stream());
    if (done != 0) return done;
    *blocks = counted.blocks;
    return 0;
}

int bsr_to_csr_gpu(CSRMatrix* A, const BSRMatrix* B, int keep_zeros) {
    return detail::bsr::to_csr(A, B, keep_zeros, detail::current_stream());
}

SpMVResult spmv_bsr(const BSRMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config, int vec_size) {
    using namespace detail;
    SpMVResult result;
    bool nothing = false;
    result.error_code = bsr::spmv_check(A, d_x, d_y, vec_size, &nothing);
    if (result.error_code != 0) return result;
    result.y = d_y;
    if (nothing) return result;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!bsr::block_size_ok(config)) {
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
        result.y = nullptr;
        return result;
    }
    const TraceRange range("spmv:spmv_bsr");
    hipStream_t stream = current_stream();
    EventPair& ev = thread_events();
    bool ok = ev.start && ev.stop && hipEventRecord(ev.start, stream) == hipSuccess;
    ok = ok && bsr::enqueue(A, d_x, d_y, config, stream) == hipSuccess;
    ok = ok && hipEventRecord(ev.stop, stream) == hipSuccess && hipEventSynchronize(ev.stop) == hipSuccess &&
         hipGetLastError() == hipSuccess && hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
        result.y = nullptr;
        return result;
    }
    if (result.elapsed_ms > 0.0f) {
        result.gflops = static_cast<float>(2.0 * A->num_blocks * A->block_dim * A->block_dim / (result.elapsed_ms * 1e6));
    }
    result.bandwidth_gb_s = compute_bandwidth_bsr(A, result.elapsed_ms).achieved_bandwidth_gb_s;
    return result;
}

int spmv_bsr_async(const BSRMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config, int vec_size,
                   hipStream_t stream) {
    using namespace detail;
    bool nothing = false;
    const int status = bsr::spmv_check(A, d_x, d_y, vec_size, &nothing);
    if (status != 0 || nothing) return status;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!bsr::block_size_ok(config)) return code(SpMVError::KERNEL_LAUNCH);
    return bsr::enqueue(A, d_x, d_y, config, stream) == hipSuccess ? code(SpMVError::SUCCESS)
                                                                   : code(SpMVError::KERNEL_LAUNCH);
}

} // namespace spmv
