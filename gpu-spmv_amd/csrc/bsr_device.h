// bsr_device.h — what the kernel files that walk a BSR matrix share (bsr.hip, cg_bsr.hip, bsr_tri.hip; DESIGN.md §4.29 -
// §4.31):
// the block-size dispatch, the lane rule of the lane-group product, the block load and the block-row walk with a
// sink, which is to BSR what for_each_row_dot (device_common.h) is to CSR.  Internal: not installed under include/.
#ifndef SPMV_AMD_BSR_DEVICE_H
#define SPMV_AMD_BSR_DEVICE_H

#include "device_common.h"
#include "internal.h"
#include "spmv/bsr_matrix.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace spmv {
namespace detail {
namespace bsr {

// Calls launch(std::integral_constant<int, B>{}) for a supported block size (bsr_block_dim_supported).
template <class Launch>
hipError_t with_block_dim(int block_dim, Launch&& launch) {
    switch (block_dim) {
        case 2:  return launch(std::integral_constant<int, 2>{});
        case 3:  return launch(std::integral_constant<int, 3>{});
        case 4:  return launch(std::integral_constant<int, 4>{});
        default: return launch(std::integral_constant<int, 8>{});
    }
}

// lanes that share a block row of `items` / block_rows items on average (SPMV_DEBUG=bsr_lanes=N forces a count)
inline int lanes_for(long long items, int block_rows) {
    if (int f = forced_lanes("bsr_lanes")) return f;
    return pick_lanes_per_row(static_cast<float>(items) / static_cast<float>(std::max(block_rows, 1)));
}

// The lane-group product's count: a lane takes a whole block per step, so the smallest group with 2 * LANES >= the
// mean blocks per block row, i.e. about two steps per block row (measured best or within 6 % of it on every stencil
// of §4.29's table).
inline int product_lanes(const BSRMatrix* A) { return lanes_for(2LL * A->num_blocks, A->num_block_rows); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the B*B values of one block: 16-byte loads (WIDE: B*B % 4 == 0 and a 16-byte aligned array), else dwords
template <int B, bool WIDE>
__device__ __forceinline__ void load_block(const float* __restrict__ block, float (&v)[B * B]) {
    if constexpr (WIDE) {
        const dev::f32x4* q = reinterpret_cast<const dev::f32x4*>(block);
#pragma unroll
        for (int k = 0; k < B * B / 4; ++k) {
            const dev::f32x4 t = q[k];
            v[4 * k] = t[0];
            v[4 * k + 1] = t[1];
            v[4 * k + 2] = t[2];
            v[4 * k + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int k = 0; k < B * B; ++k) v[k] = block[k];
    }
}

// One block row's part of the walk: lane `lane` of a group of LANES takes the blocks begin + lane, begin + lane + LANES,
// ... of [begin, end) and adds their products with x into its B accumulators.  n is the number of columns: x is not read
// at or past it.  FILTER (the triangular solves, bsr_tri.hip): only the blocks whose block column lies in [lo, hi) are
// taken, the prefix or the suffix of a block row with ascending block columns.  ORDERED: product and sum rounded
// separately (spmv_cpu_bsr's sum when LANES == 1), else fused.  x carries no __restrict__: a solve reads and writes it.
template <int B, int LANES, bool WIDE, bool FILTER = false, bool ORDERED = false>
__device__ __forceinline__ void block_row_partial_dot(const int* __restrict__ bc, const float* __restrict__ bv,
                                                      const float* x, int n, int begin, int end, int lane, int lo,
                                                      int hi, float (&acc)[B]) {
    for (int p = begin + lane; p < end; p += LANES) {
        const int J = bc[p];
        if constexpr (FILTER) {
            if (J < lo || J >= hi) continue;
        }
        const int c0 = J * B;
        float v[B * B];
        load_block<B, WIDE>(bv + static_cast<long long>(p) * (B * B), v);
        if (c0 + B <= n) {
            float xv[B];
#pragma unroll
            for (int c = 0; c < B; ++c) xv[c] = x[c0 + c];
#pragma unroll
            for (int r = 0; r < B; ++r) {
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    acc[r] = ORDERED ? __fadd_rn(acc[r], __fmul_rn(v[r * B + c], xv[c]))
                                     : __builtin_fmaf(v[r * B + c], xv[c], acc[r]);
                }
            }
        } else {                                 // the last block column of a matrix whose width is no multiple of B:
#pragma unroll                                   // positions past num_cols are skipped by select, x is not read there
            for (int c = 0; c < B; ++c) {
                const bool inside = c0 + c < n;
                const float xc = inside ? x[c0 + c] : 0.0f;
#pragma unroll
                for (int r = 0; r < B; ++r) {
                    const float next = ORDERED ? __fadd_rn(acc[r], __fmul_rn(v[r * B + c], xc))
                                               : __builtin_fmaf(v[r * B + c], xc, acc[r]);
                    acc[r] = inside ? next : acc[r];
                }
            }
        }
    }
}

// The block-row sweep: a group of LANES lanes per block row, lane l takes blocks l, l + LANES, ... of it, holds B
// accumulators, and group_sum folds each of them.  row_done(row, sum) is called for every scalar row < m with the row's
// dot product with x, by lane r % LANES of the group for row I * B + r: lanes 0 .. B-1, or every lane in turn in a
// group narrower than B.  Every lane of the workgroup makes every trip (group_sum is cross-lane), so row_done may not
// leave the kernel.  n is the number of columns: x is not read at or past it.
template <int B, int LANES, bool WIDE, class RowDone>
__device__ __forceinline__ void for_each_block_row_dot(const int* __restrict__ brp, const int* __restrict__ bc,
                                                       const float* __restrict__ bv, const float* __restrict__ x,
                                                       int m, int n, int block_rows, RowDone&& row_done) {
    constexpr int kRowsPerBlock = dev::kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < block_rows;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long I = first + slot;
        float acc[B];
#pragma unroll
        for (int r = 0; r < B; ++r) acc[r] = 0.0f;
        if (I < block_rows) block_row_partial_dot<B, LANES, WIDE>(bc, bv, x, n, brp[I], brp[I + 1], lane, 0, 0, acc);
#pragma unroll
        for (int r = 0; r < B; ++r) acc[r] = dev::group_sum<LANES>(acc[r]);
        if (I < block_rows) {
#pragma unroll
            for (int r = 0; r < B; ++r) {        // lanes 0 .. B-1 finish (a group narrower than B: lane r % LANES)
                const long long row = I * B + r;
                if (r % LANES == lane && row < m) row_done(row, acc[r]);
            }
        }
    }
}

} // namespace bsr
} // namespace detail
} // namespace spmv

#endif
