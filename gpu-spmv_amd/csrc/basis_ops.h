// basis_ops.h — the ungated device functions that walk a pitched basis of fp32 vectors: what gmres.hip's and
// eigs.hip's orthogonalisation kernels are made of.  Every function is force-inlined into the kernel that calls it;
// each solver gates its own kernels on its own state.  The basis is walked in compile-time groups of kGroup vectors
// with kGroup fp64 accumulators in registers; a thread's four elements of w stay in registers across the groups of an
// update.  No per-thread array is indexed at run time: the coefficients live in LDS.  Internal: not installed.
#ifndef SPMV_AMD_BASIS_OPS_H
#define SPMV_AMD_BASIS_OPS_H

#include "device_common.h"
#include "solver_common.h"

#include <hip/hip_runtime.h>

namespace spmv {
namespace detail {
namespace basis {

using dev::block_sum2;
using dev::f32x4;
using dev::kBlock;
using solver::prod64;

constexpr int kGroup = 8;                  // basis vectors per compile-time group
constexpr int kChunk = 4 * kBlock;         // elements of w a workgroup holds in registers at a time
constexpr int kOrthoBlocks = 256;          // workgroups of the basis kernels: every one folds (j+1) x this many partials

// a thread's four consecutive elements of one of the solver's own vectors (16-byte aligned, padded to the leading
// dimension); elements at or past n read as 0 whatever the padding holds
__device__ __forceinline__ f32x4 load4_masked(const float* v, long long e, long long n) {
    f32x4 out = {0.0f, 0.0f, 0.0f, 0.0f};
    if (e < n) {
        const f32x4 raw = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = e + q < n ? raw[q] : 0.0f;
    }
    return out;
}

__device__ __forceinline__ void store4(float* v, long long e, long long n, f32x4 val) {
    if (e < n) *reinterpret_cast<f32x4*>(v + e) = val;      // e + 3 < the leading dimension
}

__device__ __forceinline__ double dot4(f32x4 a, f32x4 b) {
    return (prod64(a[0], b[0]) + prod64(a[1], b[1])) + (prod64(a[2], b[2]) + prod64(a[3], b[3]));
}

// s_out[i] = fp32(sum over p < P of part[i * P + p]) for i < count, in a fixed order: wave (i mod 4) sums a fixed
// strided subset per lane, then a butterfly.
__device__ __forceinline__ void fold_columns(const double* __restrict__ part, int P, int count,
                                             float* __restrict__ s_out) {
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x >> 6; i < count; i += kBlock / 64) {
        double a = 0.0;
        for (int p = lane; p < P; p += 64) a += part[static_cast<long long>(i) * P + p];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) s_out[i] = static_cast<float>(a);
    }
    __syncthreads();
}

// part[i * gridDim.x + block] = this workgroup's share of v_i.w for i < nv
__device__ __forceinline__ void multidot_pass(long long n, long long ld, int nv, const float* __restrict__ V,
                                              const float* w, double* __restrict__ part) {
    for (int first = 0; first < nv; first += kGroup) {
        const int count = min(kGroup, nv - first);
        double acc[kGroup];
#pragma unroll
        for (int i = 0; i < kGroup; ++i) acc[i] = 0.0;
        for (long long base = static_cast<long long>(blockIdx.x) * kChunk; base < n;
             base += static_cast<long long>(gridDim.x) * kChunk) {
            const long long e = base + 4 * threadIdx.x;
            const f32x4 w4 = load4_masked(w, e, n);
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                if (i < count) acc[i] += dot4(w4, load4_masked(V + (first + i) * ld, e, n));
            }
        }
#pragma unroll
        for (int i = 0; i < kGroup; i += 2) {
            if (i < count) {                        // uniform over the workgroup
                block_sum2(acc[i], acc[i + 1]);
                if (threadIdx.x == 0) {
                    part[static_cast<long long>(first + i) * gridDim.x + blockIdx.x] = acc[i];
                    if (i + 1 < count) part[static_cast<long long>(first + i + 1) * gridDim.x + blockIdx.x] = acc[i + 1];
                }
            }
        }
    }
}

// w4 <- fmaf(-s_h[i], v_i, w4) for i < nv ascending, on this thread's four elements
__device__ __forceinline__ f32x4 subtract_all(long long n, long long ld, int nv, const float* __restrict__ V,
                                              const float* s_h, long long e, f32x4 w4) {
    for (int first = 0; first < nv; first += kGroup) {
        const int count = min(kGroup, nv - first);
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            if (i < count) {
                const float h = s_h[first + i];
                const f32x4 v4 = load4_masked(V + (first + i) * ld, e, n);
#pragma unroll
                for (int q = 0; q < 4; ++q) w4[q] = __builtin_fmaf(-h, v4[q], w4[q]);
            }
        }
    }
    return w4;
}

} // namespace basis
} // namespace detail
} // namespace spmv

#endif
