// multi_window.h — the row slices of the k-wide kernels (cg_multi.hip, sptrsv_multi.hip, pagerank_multi_vec.hip): W
// consecutive columns of one row of a row-major array, as 16-byte accesses where alignment and leading dimension
// allow and guarded scalar ones otherwise; and with_window, the host's pick of the kernel instantiation for a window
// width.  Internal: not installed under include/.
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

} // namespace dev

namespace solver {

// Calls launch(std::integral_constant<int, W>{}) for the window width w of a k-wide workspace: 4 (k <= 4), else 8
// (host side; with_lanes' shape, solver_common.h).
template <class Launch>
hipError_t with_window(int w, Launch&& launch) {
    if (w == 4) return launch(std::integral_constant<int, 4>{});
    return launch(std::integral_constant<int, 8>{});
}

} // namespace solver
} // namespace detail
} // namespace spmv

#endif
