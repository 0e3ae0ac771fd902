// sptrsv.hip — solve kernels of the sparse triangular solve (include/spmv/sptrsv.h).
//
// One kernel, launched per group of the schedule by the level layer of device_common.h (launch_level_groups: a grid
// per wide level, one workgroup per run of narrow levels).  The walk over the levels is for_each_level_row's, written
// out: through the helper the instantiations with more than one lane came out with another block layout and a split
// DPP add, 0.7 to 0.9 % on a preconditioned CG step (profiles/level_layer_ab.txt).  Why a level sees the previous
// level's x is said at the helper.
//
// x and b are deliberately not __restrict__: they may be the same array, and x is read and written in one launch.
#include "internal.h"
#include "device_common.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

// ORDERED (LANES == 1): the CPU's order and roundings, product then sum.  Otherwise each lane takes the entries
// begin + lane, begin + lane + LANES, ... with fused multiply-adds and the partial sums fold in group_sum's fixed
// butterfly.  Row pointers and column indices are clamped to the arrays, so a matrix whose structure was rewritten
// behind the cached schedule gives wrong numbers, never an out-of-bounds access.
template <int LANES, bool ORDERED>
__global__ __launch_bounds__(kBlock)
void sptrsv_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                   const float* __restrict__ vals, const float* b, float* x, const int* __restrict__ level_ptr,
                   const int* __restrict__ order, int level_begin, int level_end, int upper, int unit) {
    static_assert(!ORDERED || LANES == 1, "the ordered solve is one lane per row");
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (int level = level_begin; level < level_end; ++level) {
        const int first = level_ptr[level];
        const int last = min(level_ptr[level + 1], n);
        for (long long base = first + static_cast<long long>(blockIdx.x) * kRowsPerBlock; base < last;
             base += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
            const long long k = base + slot;
            const bool live = k >= 0 && k < last;
            int i = 0, begin = 0, end = 0;
            float s = 0.0f, d = 0.0f, hits = 0.0f;
            if (live) {
                i = min(max(order[k], 0), n - 1);
                begin = max(row_ptrs[i], 0);
                end = min(row_ptrs[i + 1], nnz);
                for (int j = begin + lane; j < end; j += LANES) {
                    const int c = cols[j];
                    const float v = vals[j];
                    if (c == i) {
                        d = __fadd_rn(d, v);
                        hits += 1.0f;
                    } else if (upper ? (c > i && c < n) : (static_cast<unsigned>(c) < static_cast<unsigned>(i))) {
                        const float xj = x[c];
                        s = ORDERED ? __fadd_rn(s, __fmul_rn(v, xj)) : __builtin_fmaf(v, xj, s);
                    }
                }
            }
            if constexpr (LANES > 1) {
                s = group_sum<LANES>(s);
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
            if (live && lane == 0) x[i] = __fdiv_rn(__fsub_rn(b[i], s), unit ? 1.0f : d);
        }
        if (level + 1 < level_end) __syncthreads();
    }
}

template <int LANES, bool ORDERED>
hipError_t launch_groups(const SptrsvSchedule& sch, const CSRMatrix* A, const float* b, float* x, int upper, int unit,
                         hipStream_t s) {
    return launch_level_groups<LANES>(sch, [&](int grid, int level_begin, int level_end) {
        sptrsv_kernel<LANES, ORDERED><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices,
                                                             A->d_values, b, x, sch.d_level_ptr, sch.d_order,
                                                             level_begin, level_end, upper, unit);
    });
}

} // namespace

hipError_t launch_sptrsv(const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_b, float* d_x, int uplo,
                         int unit_diagonal, bool ordered, int lanes_per_row, hipStream_t s) {
    if (ordered) return launch_groups<1, true>(schedule, A, d_b, d_x, uplo, unit_diagonal, s);
    return with_lanes(lanes_per_row, [&](auto L) {
        return launch_groups<decltype(L)::value, false>(schedule, A, d_b, d_x, uplo, unit_diagonal, s);
    });
}

} // namespace detail
} // namespace spmv
