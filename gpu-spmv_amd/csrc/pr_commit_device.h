// pr_commit_device.h — the single-rank residual commit as one device function, shared by
// pr_reduce_commit_kernel (pagerank.hip) and the commit workgroup at the head of a phase-1
// launch (tiled.hip), so that both forms produce the same bits.
#ifndef SPMV_AMD_PR_COMMIT_DEVICE_H
#define SPMV_AMD_PR_COMMIT_DEVICE_H

#include "device_common.h"
#include "pagerank_engine.h"

namespace spmv {
namespace detail {
namespace dev {

// Folds the block partials left to right (thread t takes t, t + kBlock, ...; then block_sum2) and applies them:
// residual, iteration count, convergence flag, dangling mass for the next step.  Called by the first kBlock
// threads of a workgroup, all of them; whole wavefronts past kBlock must have left before.
__device__ __forceinline__ void pr_fold_and_commit(const double* __restrict__ block_partials, int num_blocks,
                                                   float tolerance, PrState* __restrict__ state) {
    if (state->done) return;
    double res2 = 0.0, mass = 0.0;
    for (int b = threadIdx.x; b < num_blocks; b += kBlock) {
        res2 += block_partials[2 * b];
        mass += block_partials[2 * b + 1];
    }
    block_sum2(res2, mass);
    if (threadIdx.x == 0) {
        const float residual = static_cast<float>(sqrt(res2));
        state->iterations += 1;
        state->final_residual = residual;
        state->dangling_sum = static_cast<float>(mass);
        if (residual < tolerance) {
            state->converged = 1;
            state->done = 1;
        }
    }
}

} // namespace dev
} // namespace detail
} // namespace spmv

#endif
