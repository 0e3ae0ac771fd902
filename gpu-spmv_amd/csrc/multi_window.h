// multi_window.h — what the k-wide kernels (cg_multi.hip, sptrsv_multi.hip, pagerank_multi_vec.hip) share.
//   row slices   W consecutive columns of one row of a row-major array, as 16-byte accesses where alignment and
//                leading dimension allow and guarded scalar ones otherwise: load_window, load_own / store_own,
//                load_window_shared / store_window
//   the row sum  row_partial_dot_multi: row_partial_dot's walk with W accumulators
//   reductions   block_sum_columns and fold_values: block_sum2's workgroup sum for N values behind two barriers
//   with_window  the host's pick of the kernel instantiation for a window width
// Internal: not installed under include/.
#ifndef SPMV_AMD_MULTI_WINDOW_H
#define SPMV_AMD_MULTI_WINDOW_H

#include "device_common.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace spmv {
namespace detail {
namespace dev {

// W floats of row `row` of the row-major array V (leading dimension ld), from column j0 (a multiple of 4) on;
// columns at or past `limit` come back 0.  vec: V is 16-byte aligned and ld % 4 == 0, so every group of four
// columns that lies below `limit` loads as dwordx4; the rest are guarded scalar loads.
template <int W>
__device__ __forceinline__ void load_window(const float* __restrict__ V, long long ld, long long row, int j0,
                                            int limit, bool vec, float (&out)[W]) {
    const float* p = V + row * ld + j0;
#pragma unroll
    for (int g = 0; g < W; g += 4) {
        if (vec && j0 + g + 4 <= limit) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + g);
            out[g] = v[0]; out[g + 1] = v[1]; out[g + 2] = v[2]; out[g + 3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) out[g + e] = j0 + g + e < limit ? p[g + e] : 0.0f;
        }
    }
}

// load_window on the solver's own arrays: they are 16-byte aligned with ld a multiple of 4 and padded to ld, so every
// group of four columns below ld loads as dwordx4 (the padding columns hold nothing that is ever used).  The loop
// kernels pass one window (ld = W, j0 = 0): W / 4 unconditional loads.
template <int W>
__device__ __forceinline__ void load_own(const float* __restrict__ V, long long ld, long long row, int j0,
                                         float (&out)[W]) {
    const float* p = V + row * ld + j0;
#pragma unroll
    for (int g = 0; g < W; g += 4) {
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j0 + g < ld) v = *reinterpret_cast<const f32x4*>(p + g);
        out[g] = v[0]; out[g + 1] = v[1]; out[g + 2] = v[2]; out[g + 3] = v[3];
    }
}

// The store that goes with load_own's one-window case: row `row` of one of the solver's own windows (num_rows x W,
// 16-byte aligned, ld = W) as W / 4 unconditional dwordx4 stores.
template <int W>
__device__ __forceinline__ void store_own(float* __restrict__ window, long long row, const float (&in)[W]) {
    float* p = window + row * W;
#pragma unroll
    for (int g = 0; g < W; g += 4) {
        const f32x4 v = {in[g], in[g + 1], in[g + 2], in[g + 3]};
        *reinterpret_cast<f32x4*>(p + g) = v;
    }
}

// load_window without the __restrict__ promise, for an array that the same launch also writes (sptrsv_multi.hip's X,
// which B may alias), from the window's first column on (limit >= 1 columns exist).  A column at or past `limit`
// comes back as a copy of column limit - 1 instead of 0: the scalar loads clamp their column where load_window
// guards it (one scalar register per column instead of a condition pair), and the caller never stores such a column.
template <int W>
__device__ __forceinline__ void load_window_shared(const float* V, int ld, int row, int limit, bool vec,
                                                   float (&out)[W]) {
    const float* p = V + static_cast<long long>(row) * ld;
#pragma unroll
    for (int g = 0; g < W; g += 4) {
        if (vec && g + 4 <= limit) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + g);
            out[g] = v[0]; out[g + 1] = v[1]; out[g + 2] = v[2]; out[g + 3] = v[3];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) out[g + e] = p[min(g + e, limit - 1)];
        }
    }
}

// The store that goes with load_window_shared: columns at or past `limit` are not written.
template <int W>
__device__ __forceinline__ void store_window(float* V, int ld, int row, int limit, bool vec,
                                             const float (&in)[W]) {
    float* p = V + static_cast<long long>(row) * ld;
#pragma unroll
    for (int g = 0; g < W; g += 4) {
        if (vec && g + 4 <= limit) {
            const f32x4 v = {in[g], in[g + 1], in[g + 2], in[g + 3]};
            *reinterpret_cast<f32x4*>(p + g) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (g + e < limit) p[g + e] = in[g + e];
            }
        }
    }
}

// block_sum2's sum of N values at once behind two barriers in all: the same xor butterfly inside each wavefront,
// then the wavefronts' totals added in wave order, so thread c (< N) returns for v[c] the very bits block_sum2 leaves
// in thread 0.  Other threads return 0.
template <int N>
__device__ __forceinline__ double block_sum_columns(double (&v)[N]) {
    static_assert(N <= kBlock, "one thread per value");
    __shared__ double s_wave[kBlock / 64][N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) s_wave[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x < N) {
        total = s_wave[0][threadIdx.x];
        for (int w = 1; w < kBlock / 64; ++w) total += s_wave[w][threadIdx.x];
    }
    __syncthreads();
    return total;
}

// The second half of fold_partials (solver_common.h) and of pr_fold_and_commit for N values at once: v[c] holds this
// thread's strided sum (i = threadIdx.x, threadIdx.x + 256, ... in that order, as they add them); the same butterfly
// and wave order as block_sum2, and every thread leaves with the totals.  Two barriers for N values where
// fold_partials takes four for a pair.
template <int N>
__device__ __forceinline__ void fold_values(double (&v)[N]) {
    __shared__ double s_wave[kBlock / 64][N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) s_wave[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        v[c] = s_wave[0][c];
        for (int w = 1; w < kBlock / 64; ++w) v[c] += s_wave[w][c];
    }
    __syncthreads();
}

// row_partial_dot<LANES> with W accumulators: the same walk (start, stride, load4, select-masked neighbours) and,
// per column, the same fmaf chain; every entry's slice V[c, j0 : j0 + W] is loaded once.  OWN: V is one of the
// solver's own arrays (load_own; limit and vec are not read).
template <int LANES, int W, bool OWN>
__device__ __forceinline__ void row_partial_dot_multi(int begin, int end, int lane, long long nnz,
                                                      const int* __restrict__ cols, const float* __restrict__ vals,
                                                      const float* __restrict__ V, long long ld, int j0, int limit,
                                                      bool vec, float (&acc)[W]) {
    for (long long j = (begin & ~3) + lane * 4; j < end; j += LANES * 4) {
        i32x4 c;
        f32x4 v;
        load4(cols, vals, j, nnz, c, v);
        bool mine[4];
        float xv[4][W];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mine[e] = j + e >= begin && j + e < end;
            if constexpr (OWN) load_own<W>(V, ld, mine[e] ? c[e] : 0, j0, xv[e]);
            else load_window<W>(V, ld, mine[e] ? c[e] : 0, j0, limit, vec, xv[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int q = 0; q < W; ++q) acc[q] = mine[e] ? __builtin_fmaf(v[e], xv[e][q], acc[q]) : acc[q];
        }
    }
}

} // namespace dev

namespace solver {

// Calls launch(std::integral_constant<int, W>{}) for the window width w of a k-wide workspace: 4 (k <= 4), else 8
// (host side; with_lanes' shape, device_common.h).
template <class Launch>
hipError_t with_window(int w, Launch&& launch) {
    if (w == 4) return launch(std::integral_constant<int, 4>{});
    return launch(std::integral_constant<int, 8>{});
}

} // namespace solver
} // namespace detail
} // namespace spmv

#endif
