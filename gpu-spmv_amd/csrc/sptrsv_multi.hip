// sptrsv_multi.hip — the sparse triangular solve for k right-hand sides in one launch sequence
// (include/spmv/sptrsv.h sptrsv_csr_multi).
//
// sptrsv.hip's kernel, k-wide: the same schedule, the same launches (device_common.h launch_level_groups), the same
// walk over the levels, written out as there (through for_each_level_row the W = 8 kernels measured 0.4 to 0.5 %
// slower on the upper solves: profiles/level_layer_ab.txt), the same clamps of row pointers, column indices and the
// order array.
// A lane keeps W accumulators (4 up to k = 4, else 8; 4 at 32 and 64 lanes per row), walks the entries begin + lane,
// begin + lane + LANES, ... as the single kernel does, loads the slice X[c, j0 : j0 + W] of each entry once and
// applies the single kernel's operation per column in entry order; the partial sums fold with group_sum<LANES> per
// accumulator.  So column j is bit for bit sptrsv_kernel<LANES, ORDERED> on that column.  For k > W the further
// windows are visited inside the row (its entries come from cache then): a level stays one launch.  The diagonal is
// summed in the first window's walk and kept.
//
// One addressing rule serves the caller's arrays and the windowed workspace of cg_multi.hip: column c of row i lives
// at base + (c / WS) * window + i * ld + c % WS, WS = 4 or 8 the layout's window.  A caller's num_rows x k array has
// window = WS; the workspace's arrays (num_rows x WS one after another) have window = num_rows * WS and ld = WS.
//
// X and B are deliberately not __restrict__: they may be the same array, and X is read and written in one launch.  In
// place, a row reads window w of B before it writes window w of X, and no other row or window touches those addresses.
#include "internal.h"
#include "device_common.h"
#include "multi_window.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

// the kernel's `flags`: which triangle, the diagonal mode, and whether B / X take 16-byte accesses
constexpr int kUpper = 1, kUnit = 2, kVecB = 4, kVecX = 8;

// W: accumulators per lane; WS: columns per window of the layout (W divides WS).
template <int LANES, int W, int WS, bool ORDERED>
__global__ __launch_bounds__(kBlock)
void sptrsv_multi_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                         const float* __restrict__ vals, const float* B, int ldb, long long b_window, float* X, int ldx,
                         long long x_window, int k, const int* __restrict__ level_ptr,
                         const int* __restrict__ order, int level_begin, int level_end, int flags) {
    static_assert(!ORDERED || LANES == 1, "the ordered solve is one lane per row");
    static_assert(W % 4 == 0 && WS % W == 0, "windows are whole groups of four columns");
    constexpr int kRowsPerBlock = kBlock / LANES;
    const bool upper = flags & kUpper, unit = flags & kUnit, b_vec = flags & kVecB, x_vec = flags & kVecX;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (int level = level_begin; level < level_end; ++level) {
        const int first = level_ptr[level];
        const int last = min(level_ptr[level + 1], n);
        for (long long base = first + static_cast<long long>(blockIdx.x) * kRowsPerBlock; base < last;
             base += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
            const long long pos = base + slot;
            const bool live = pos >= 0 && pos < last;
            int i = 0, begin = 0, end = 0;
            float d = 0.0f, hits = 0.0f;
            if (live) {
                i = min(max(order[pos], 0), n - 1);
                begin = max(row_ptrs[i], 0);
                end = min(row_ptrs[i + 1], nnz);
            }
            for (int j0 = 0; j0 < k; j0 += W) {
                const int limit = k - j0;                       // columns of this window that exist (may exceed W)
                const float* bw = B + (j0 / WS) * b_window + j0 % WS;
                float* xw = X + (j0 / WS) * x_window + j0 % WS;
                float s[W];
#pragma unroll
                for (int q = 0; q < W; ++q) s[q] = 0.0f;
                if (live) {
                    for (int j = begin + lane; j < end; j += LANES) {
                        const int c = cols[j];
                        const float v = vals[j];
                        if (c == i) {
                            if (j0 == 0) {
                                d = __fadd_rn(d, v);
                                hits += 1.0f;
                            }
                        } else if (upper ? (c > i && c < n) : (static_cast<unsigned>(c) < static_cast<unsigned>(i))) {
                            float xj[W];
                            load_window_shared<W>(xw, ldx, c, limit, x_vec, xj);
#pragma unroll
                            for (int q = 0; q < W; ++q) {
                                s[q] = ORDERED ? __fadd_rn(s[q], __fmul_rn(v, xj[q])) : __builtin_fmaf(v, xj[q], s[q]);
                            }
                        }
                    }
                }
                if constexpr (LANES > 1) {
#pragma unroll
                    for (int q = 0; q < W; ++q) s[q] = group_sum<LANES>(s[q]);
                    if (j0 == 0) {
                        d = group_sum<LANES>(d);
                        hits = group_sum<LANES>(hits);
                        // one or two diagonal entries fold to the storage-order sum whatever the lanes; more are rare:
                        // lane 0 adds them up again in storage order
                        if (live && lane == 0 && !unit && hits > 2.0f) {
                            d = 0.0f;
                            for (int j = begin; j < end; ++j) {
                                if (cols[j] == i) d = __fadd_rn(d, vals[j]);
                            }
                        }
                    }
                }
                if (live && lane == 0) {
                    float bi[W], xi[W];
                    load_window_shared<W>(bw, ldb, i, limit, b_vec, bi);
                    const float di = unit ? 1.0f : d;
#pragma unroll
                    for (int q = 0; q < W; ++q) xi[q] = __fdiv_rn(__fsub_rn(bi[q], s[q]), di);
                    store_window<W>(xw, ldx, i, limit, x_vec, xi);
                }
            }
        }
        if (level + 1 < level_end) __syncthreads();
    }
}

template <int LANES, int W, int WS, bool ORDERED>
hipError_t launch_groups(const SptrsvSchedule& sch, const CSRMatrix* A, const SptrsvMultiArrays& a, int upper,
                         int unit, hipStream_t s) {
    // 16-byte accesses: the base and every window and row offset are multiples of 16 bytes
    const auto vec = [](const float* p, long long ld, long long window) {
        return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0 && window % 4 == 0;
    };
    const int flags = (upper ? kUpper : 0) | (unit ? kUnit : 0) | (vec(a.B, a.ldb, a.b_window) ? kVecB : 0) |
                      (vec(a.X, a.ldx, a.x_window) ? kVecX : 0);
    return launch_level_groups<LANES>(sch, [&](int grid, int level_begin, int level_end) {
        sptrsv_multi_kernel<LANES, W, WS, ORDERED><<<grid, kBlock, 0, s>>>(
            A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, a.B, a.ldb, a.b_window, a.X, a.ldx,
            a.x_window, a.k, sch.d_level_ptr, sch.d_order, level_begin, level_end, flags);
    });
}

// WS: the layout's window.  Eight accumulators per lane at 32 and 64 lanes per row push scalar registers out (the
// butterfly's extra steps on top of the window's guards): those two take the window of eight in two halves of four.
template <int WS>
hipError_t launch_width(const SptrsvSchedule& schedule, const CSRMatrix* A, const SptrsvMultiArrays& a, int uplo,
                        int unit_diagonal, bool ordered, int lanes_per_row, hipStream_t s) {
    if (ordered) return launch_groups<1, WS, WS, true>(schedule, A, a, uplo, unit_diagonal, s);
    return with_lanes(lanes_per_row, [&](auto L) {
        constexpr int kLanes = decltype(L)::value;
        constexpr int kW = kLanes >= 32 ? 4 : WS;
        return launch_groups<kLanes, kW, WS, false>(schedule, A, a, uplo, unit_diagonal, s);
    });
}

} // namespace

hipError_t launch_sptrsv_multi(const SptrsvSchedule& schedule, const CSRMatrix* A, const SptrsvMultiArrays& arrays,
                               int uplo, int unit_diagonal, bool ordered, int lanes_per_row, hipStream_t s) {
    if (arrays.w == 4) return launch_width<4>(schedule, A, arrays, uplo, unit_diagonal, ordered, lanes_per_row, s);
    return launch_width<8>(schedule, A, arrays, uplo, unit_diagonal, ordered, lanes_per_row, s);
}

} // namespace detail
} // namespace spmv
