// solver_common.h — pieces shared by the device-resident Krylov solvers (cg.hip, bicgstab.hip): the deterministic
// fp64 dot-product partials and their fixed-order fold, the grid sizes, the LANES dispatch of the vector-CSR
// kernels, the b / x overlap check and the workspace of one solve.  Internal: not installed under include/.
#ifndef SPMV_AMD_SOLVER_COMMON_H
#define SPMV_AMD_SOLVER_COMMON_H

#include "device_common.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace spmv {
namespace detail {
namespace solver {

using dev::kBlock;
using dev::kMaxResidentBlocks;

constexpr int kVecBlocks = 1024;      // workgroups of the element-wise kernels (4 per CU)

// Sums part[i * stride] (and part[i * stride + 1] when stride > 1 and `pair`) over i < count in a fixed order,
// broadcast to every thread: each thread folds a fixed strided subset, then block_sum2's fixed butterfly and wave
// order.  pair = false reads nothing but part[i * stride] (b comes back 0): for a single value per group whose
// neighbour may lie past the end of the array.
__device__ __forceinline__ void fold_partials(const double* __restrict__ part, int count, int stride,
                                              double& a, double& b, bool pair = true) {
    __shared__ double s_fold[2];
    a = 0.0;
    b = 0.0;
    for (int i = threadIdx.x; i < count; i += kBlock) {
        a += part[static_cast<long long>(i) * stride];
        if (stride > 1 && pair) b += part[static_cast<long long>(i) * stride + 1];
    }
    dev::block_sum2(a, b);
    if (threadIdx.x == 0) {
        s_fold[0] = a;
        s_fold[1] = b;
    }
    __syncthreads();
    a = s_fold[0];
    b = s_fold[1];
}

__device__ __forceinline__ double prod64(float a, float b) {
    return static_cast<double>(a) * static_cast<double>(b);   // exact: 24 + 24 bits fit in fp64
}

inline int grid_for_rows(long long rows, int rows_per_block) {
    const long long blocks = (rows + rows_per_block - 1) / rows_per_block;
    return static_cast<int>(std::max(1LL, std::min<long long>(blocks, kMaxResidentBlocks)));
}

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

inline bool ranges_overlap(const float* a, const float* b, long long n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = static_cast<uintptr_t>(n) * sizeof(float);
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

// Device memory of one solve, freed on every exit.  State is the solver's device state.
template <class State>
struct Workspace {
    float* vec = nullptr;          // the solver's n-float vectors
    double* part = nullptr;        // partial sums
    State* state = nullptr;
    State* pinned = nullptr;       // [2] pinned host mirror
    hipEvent_t seen[2] = {nullptr, nullptr};

    // false (and the HIP error cleared) when any allocation fails
    bool allocate(size_t vec_floats, size_t part_doubles) {
        const bool ok = hipMalloc(reinterpret_cast<void**>(&vec), vec_floats * sizeof(float)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&part), part_doubles * sizeof(double)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&state), sizeof(State)) == hipSuccess &&
                        hipHostMalloc(reinterpret_cast<void**>(&pinned), 2 * sizeof(State)) == hipSuccess &&
                        hipEventCreateWithFlags(&seen[0], hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&seen[1], hipEventDisableTiming) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    ~Workspace() {
        if (vec) (void)hipFree(vec);
        if (part) (void)hipFree(part);
        if (state) (void)hipFree(state);
        if (pinned) (void)hipHostFree(pinned);
        for (hipEvent_t e : seen) if (e) (void)hipEventDestroy(e);
    }
};

} // namespace solver
} // namespace detail
} // namespace spmv

#endif
