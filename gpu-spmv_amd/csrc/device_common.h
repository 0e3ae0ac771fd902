// device_common.h — what the kernel files share (gfx950, wave64).
// Device side: cross-lane and workgroup reductions, the vector-CSR row walk
// (row_partial_dot) and the sweep over all rows built on it (for_each_row_dot),
// the walk over the rows of a level schedule (for_each_level_row), the binary
// searches.
// Host side, the launch layer: the grid sizes (capped_grid, vec_grid),
// with_lanes, which turns a run-time lanes-per-row count into a template
// argument, and launch_level_groups, the launches of one pass over a level
// schedule.
#ifndef SPMV_AMD_DEVICE_COMMON_H
#define SPMV_AMD_DEVICE_COMMON_H

#include "internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

namespace spmv {
namespace detail {
namespace dev {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int   i32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;          // 4 wavefronts per workgroup
constexpr int kMaxResidentBlocks = 256 * 8;   // 256 CUs x 8 workgroups of 256 threads

// ---------------------------------------------------------------------------
// cross-lane helpers (DPP inside 16-lane rows, ds_bpermute across rows)
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float,
        __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// Sum over an aligned group of LANES consecutive lanes; every lane of the
// group ends up with the total (butterfly: quad perms, half-mirror, mirror,
// then xor-16 / xor-32 across DPP rows).
template <int LANES>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (LANES >= 2)  v += dpp<0xB1>(v);    // quad_perm [1,0,3,2]
    if constexpr (LANES >= 4)  v += dpp<0x4E>(v);    // quad_perm [2,3,0,1]
    if constexpr (LANES >= 8)  v += dpp<0x141>(v);   // row_half_mirror
    if constexpr (LANES >= 16) v += dpp<0x140>(v);   // row_mirror
    if constexpr (LANES >= 32) v += __shfl_xor(v, 16, 64);
    if constexpr (LANES >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u(unsigned v) {
    return static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, true));
}

// OR over an aligned group of LANES consecutive lanes, every lane gets the result (group_sum's butterfly)
template <int LANES>
__device__ __forceinline__ unsigned group_or(unsigned v) {
    if constexpr (LANES >= 2)  v |= dpp_u<0xB1>(v);
    if constexpr (LANES >= 4)  v |= dpp_u<0x4E>(v);
    if constexpr (LANES >= 8)  v |= dpp_u<0x141>(v);
    if constexpr (LANES >= 16) v |= dpp_u<0x140>(v);
    if constexpr (LANES >= 32) v |= static_cast<unsigned>(__shfl_xor(static_cast<int>(v), 16, 64));
    if constexpr (LANES >= 64) v |= static_cast<unsigned>(__shfl_xor(static_cast<int>(v), 32, 64));
    return v;
}

// inclusive prefix sum over the 64 lanes of a wavefront: Hillis-Steele inside each 16-lane DPP row
// (row_shr 1, 2, 4, 8; lanes shifted in from outside the row contribute 0), then the classic wave64 tail:
// row_bcast:15 adds lane 15 of the previous row into rows 1 and 3, row_bcast:31 adds lane 31 into rows 2, 3
__device__ __forceinline__ int wave_inclusive_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return v;
}

// 16-byte loads of four consecutive entries; the tail of the arrays (fewer
// than four entries left) falls back to guarded scalar loads so nothing is
// read past nnz.
__device__ __forceinline__ void load4(const int* __restrict__ cols, const float* __restrict__ vals,
                                      long long j, long long nnz, i32x4& c, f32x4& v) {
    if (j + 3 < nnz) {
        c = *reinterpret_cast<const i32x4*>(cols + j);
        v = *reinterpret_cast<const f32x4*>(vals + j);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = j + k < nnz;
            c[k] = ok ? cols[j + k] : 0;
            v[k] = ok ? vals[j + k] : 0.0f;
        }
    }
}

// Dot product of CSR row [begin, end) with x, spread over an aligned group of
// LANES lanes: four entries per lane per step through 16-byte aligned loads.
// Returns this lane's partial sum (reduce with group_sum<LANES>).
template <int LANES>
__device__ __forceinline__ float row_partial_dot(int begin, int end, int lane, long long nnz,
                                                 const int* __restrict__ cols,
                                                 const float* __restrict__ vals,
                                                 const float* __restrict__ x) {
    float acc = 0.0f;
    // start at the 16-byte boundary at or below `begin`
    for (long long j = (begin & ~3) + lane * 4; j < end; j += LANES * 4) {
        i32x4 c;
        f32x4 v;
        load4(cols, vals, j, nnz, c, v);
        // entries outside [begin, end) belong to neighbouring rows: masked by
        // select (not multiply-by-zero: x may hold inf / nan elsewhere)
        bool mine[4];
        float xv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mine[k] = j + k >= begin && j + k < end;
            xv[k] = x[mine[k] ? c[k] : 0];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            acc = mine[k] ? __builtin_fmaf(v[k], xv[k], acc) : acc;
        }
    }
    return acc;
}

// The vector-CSR sweep: the workgroup's aligned groups of LANES lanes stride over the rows, BLOCK / LANES rows per
// workgroup and trip; row_done(row, sum) is called by lane 0 of each group, for rows < n only, with the row's dot
// product with x (the group_sum of row_partial_dot).  Every lane of the workgroup makes every trip (group_sum is
// cross-lane), so row_done may not leave the kernel.  BLOCK is the workgroup's size.
template <int LANES, int BLOCK = kBlock, class RowDone>
__device__ __forceinline__ void for_each_row_dot(int n, long long nnz, const int* __restrict__ row_ptrs,
                                                 const int* __restrict__ cols, const float* __restrict__ vals,
                                                 const float* __restrict__ x, RowDone&& row_done) {
    constexpr int kRowsPerBlock = BLOCK / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < n;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long row = first + slot;
        float acc = 0.0f;
        if (row < n) acc = row_partial_dot<LANES>(row_ptrs[row], row_ptrs[row + 1], lane, nnz, cols, vals, x);
        acc = group_sum<LANES>(acc);
        if (lane == 0 && row < n) row_done(row, acc);
    }
}

// The level layer, device side: the walk over the levels [level_begin, level_end) of a level schedule (SptrsvSchedule:
// order[level_ptr[l] .. level_ptr[l + 1]) are the rows of level l, independent of each other), one aligned group of
// LANES lanes per row, kBlock / LANES rows per workgroup and trip.  launch_level_groups below launches it in two shapes:
//   * one wide level: a grid strides over the level's rows;
//   * a run of narrow levels (each at most kSptrsvNarrowRows rows): ONE workgroup walks them in order with
//     __syncthreads() in between (none after the last).  __syncthreads() is a workgroup-scope release, the barrier, and
//     a workgroup-scope acquire; the waves of a workgroup share their CU's vector L1, which their own write-through
//     stores keep current, so what a level stored is what the next level's plain loads return.  (Another CU would need
//     an agent-scope acquire; nothing reads another workgroup's stores inside a launch.)
// The order between launches is stream order.  No workgroup waits for another one: no flags, no spinning.
// Every thread calls body(live, row, lane) on every trip, so that body may use cross-lane operations and every thread
// reaches every barrier: body may not leave the kernel.  live: the group has a row; row() is order[] clamped to
// [0, rows), so a schedule that went stale gives wrong numbers, never an out-of-bounds access.  A dead group does not
// read order[] and gets row 0.  A body that writes `if (!live) return;` is sound: the whole LANES group leaves
// together, no shuffle reads it.
// Call row() inside the body's own `if (live)` and capture by value ([=]): every other form costs registers
// (profiles/level_layer_resources.txt).  The block kernels of bsr_tri.hip walk through this helper; sptrsv_kernel,
// sptrsv_multi_kernel and factor0_kernel write the same walk out: through the helper they measured 0.4 to 0.9 % slower
// with equal resources (profiles/level_layer_ab.txt).  A change here is a change there.
template <int LANES, class Body>
__device__ __forceinline__ void for_each_level_row(const int* level_ptr, const int* order, int level_begin,
                                                   int level_end, int rows, Body&& body) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (int level = level_begin; level < level_end; ++level) {
        const int first = level_ptr[level];
        const int last = min(level_ptr[level + 1], rows);
        for (long long base = first + static_cast<long long>(blockIdx.x) * kRowsPerBlock; base < last;
             base += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
            const long long k = base + slot;
            const bool live = k >= 0 && k < last;
            body(live, [&] { return live ? min(max(order[k], 0), rows - 1) : 0; }, lane);
        }
        if (level + 1 < level_end) __syncthreads();
    }
}

// block-wide sum of two doubles; result valid in thread 0
template <int BLOCK = kBlock>
__device__ __forceinline__ void block_sum2(double& a, double& b) {
    __shared__ double s_a[BLOCK / 64];
    __shared__ double s_b[BLOCK / 64];
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_a[wave] = a;
        s_b[wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = s_a[0];
        b = s_b[0];
        for (int w = 1; w < BLOCK / 64; ++w) {
            a += s_a[w];
            b += s_b[w];
        }
    }
    __syncthreads();
}

// Integer reduction over the workgroup by op (min, max: associative and commutative, so the order does not show):
// the xor butterfly inside each wavefront, one LDS word per wavefront, and thread 0 folds the other wavefronts' words
// into its own.  The result is valid in thread 0 ONLY, and there is no second barrier: two calls in one kernel need a
// __syncthreads() between them, or the second call's LDS stores race with thread 0's loads of the first.
template <class Op>
__device__ __forceinline__ int block_reduce_int(int v, Op op) {
    __shared__ int s_wave[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) v = op(v, s_wave[w]);
    }
    return v;
}
__device__ __forceinline__ int block_min(int v) {
    return block_reduce_int(v, [](int a, int b) { return min(a, b); });
}
__device__ __forceinline__ int block_max(int v) {
    return block_reduce_int(v, [](int a, int b) { return max(a, b); });
}

// ---------------------------------------------------------------------------
// binary searches in sorted int arrays
// ---------------------------------------------------------------------------
// position of column `want` in cols[lo, hi) (strictly ascending), or -1
__device__ __forceinline__ int find_column(const int* __restrict__ cols, int lo, int hi, int want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int c = cols[mid];
        if (c == want) return mid;
        if (c < want) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// first index j in [lo, hi) with rp[j] > p (hi when there is none)
__device__ __forceinline__ int upper_bound(const int* __restrict__ rp, int lo, int hi, long long p) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rp[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// host side: the launch layer
// ---------------------------------------------------------------------------
// workgroups for work_items at per_block each, at least one and at most `cap`: what the chip holds at once unless the
// caller has a reason for fewer (the kernels stride over the rest)
inline int capped_grid(long long work_items, int per_block, int cap = kMaxResidentBlocks) {
    const long long blocks = (work_items + per_block - 1) / per_block;
    return static_cast<int>(std::max(1LL, std::min<long long>(blocks, cap)));
}

constexpr int kVecBlocks = 1024;      // workgroups of the element-wise kernels (4 per CU)

inline int vec_grid(long long n) {
    return static_cast<int>(std::max(1LL, std::min<long long>((n + kBlock - 1) / kBlock, kVecBlocks)));
}

// Calls launch(std::integral_constant<int, LANES>{}) for the LANES pick_lanes_per_row chose (64 for anything else).
template <class Launch>
hipError_t with_lanes(int lanes, Launch&& launch) {
    switch (lanes) {
        case 1:  return launch(std::integral_constant<int, 1>{});
        case 2:  return launch(std::integral_constant<int, 2>{});
        case 4:  return launch(std::integral_constant<int, 4>{});
        case 8:  return launch(std::integral_constant<int, 8>{});
        case 16: return launch(std::integral_constant<int, 16>{});
        case 32: return launch(std::integral_constant<int, 32>{});
        default: return launch(std::integral_constant<int, 64>{});
    }
}

// The level layer, host side: one launch per group of the schedule, in stream order; launch(grid, level_begin,
// level_end) starts a kernel that walks those levels with for_each_level_row<LANES>.  The first error ends it.
template <int LANES, class Launch>
hipError_t launch_level_groups(const SptrsvSchedule& schedule, Launch&& launch) {
    for (const SptrsvSchedule::Group& g : schedule.groups) {
        // a run of levels is one workgroup (the barrier is its only ordering); one level alone takes a grid
        const int grid = g.level_end - g.level_begin > 1 ? 1 : capped_grid(g.rows, kBlock / LANES);
        launch(grid, g.level_begin, g.level_end);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace dev
} // namespace detail
} // namespace spmv

#endif
