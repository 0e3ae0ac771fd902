// cg_impl.h — what the CG kernel files (cg.hip, cg_bsr.hip) share: the device state of one solve and the four
// kernels that do not depend on the matrix format — the start of the state, the update of x and r, the r.z partials
// of a stored z and the direction step.  The kernels sit in an unnamed namespace, as they did in cg.hip: each file
// that includes this header gets its own copy under the same name, and nothing else can call them.  Internal: not
// installed under include/.
#ifndef SPMV_AMD_CG_IMPL_H
#define SPMV_AMD_CG_IMPL_H

#include "device_common.h"
#include "solver_common.h"

#include <hip/hip_runtime.h>

namespace spmv {
namespace detail {

namespace {

// Lives in device memory; every loop kernel reads `done` first.  rz is double-buffered by step parity: step k
// reads rz[k & 1] and its direction kernel writes rz[(k + 1) & 1], so no workgroup reads a slot another is writing.
struct CgState {
    double rz[2];             // r.z of the current residual
    double bnorm;             // ||b||_2
    double threshold;         // tolerance * ||b||_2
    float  relative_residual; // ||r||_2 / ||b||_2 of the last committed step
    int    iterations;        // committed steps
    int    converged;
    int    breakdown;
    int    done;              // steps after this are no-ops
    int    zero_b;            // ||b|| == 0: the host writes x = 0
    int    bad_diagonal;      // JACOBI, IC, BLOCK_JACOBI: a diagonal (block) is missing or not > 0 (IC, blocks: or not finite)
    int    reserved;
};

// One workgroup: folds the init partials and sets up the state (rz[0], ||b||, the threshold, step-0 outcome).
__global__ __launch_bounds__(dev::kBlock)
void cg_start_kernel(const double* __restrict__ part, int count, float tolerance, CgState* __restrict__ state) {
    double rz = 0.0, rr = 0.0, bb = 0.0;
    solver::fold_partials(part, count, 3, rz, rr);
    double unused = 0.0;
    solver::fold_partials(part + 2, count, 3, bb, unused, false);    // part[3 * count] is past the end: b.b alone
    if (threadIdx.x != 0) return;
    const double bnorm = sqrt(bb);
    const double res = sqrt(rr);
    state->rz[0] = rz;
    state->bnorm = bnorm;
    state->threshold = static_cast<double>(tolerance) * bnorm;
    state->iterations = 0;
    if (bb == 0.0) {
        state->zero_b = 1;
        state->relative_residual = 0.0f;
        state->converged = 1;
        state->done = 1;
        return;
    }
    state->relative_residual = static_cast<float>(res / bnorm);
    if (res <= state->threshold) {
        state->converged = 1;
        state->done = 1;
    } else if (!(rz > 0.0)) {
        state->breakdown = 1;
        state->done = 1;
    }
}

// beta = rz_new / rz_old, the stop test, p = z + beta p.  Workgroup 0 commits the step to the state.  zr is r and
// z = r * dinv (r where dinv is null), or with STORED_Z it is z itself and dinv is not read.
template <bool STORED_Z>
__global__ __launch_bounds__(dev::kBlock)
void cg_direction_kernel(int n, int step, const float* __restrict__ zr, const float* __restrict__ dinv,
                         float* __restrict__ p, CgState* __restrict__ state, const double* __restrict__ part,
                         int count) {
    if (state->done) return;
    double rz = 0.0, rr = 0.0;
    solver::fold_partials(part, count, 2, rz, rr);
    const double res = sqrt(rr);
    const bool converged = res <= state->threshold;
    const bool breakdown = !converged && !(rz > 0.0);
    const double rz_old = state->rz[step & 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->iterations = step + 1;
        state->relative_residual = static_cast<float>(res / state->bnorm);
        state->rz[(step + 1) & 1] = rz;
        if (converged) state->converged = 1;
        if (breakdown) state->breakdown = 1;
        if (converged || breakdown) state->done = 1;
    }
    if (converged || breakdown) return;
    const float beta = static_cast<float>(rz / rz_old);
    for (long long i = static_cast<long long>(blockIdx.x) * dev::kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * dev::kBlock) {
        float zi = zr[i];
        if constexpr (!STORED_Z) zi = dinv ? __fmul_rn(zi, dinv[i]) : zi;
        p[i] = __builtin_fmaf(beta, p[i], zi);
    }
}

// alpha = rz / p.q; x += alpha p; r -= alpha q; partials of r.z and r.r -> part_out[2 * block] with z = r * dinv
// (r where dinv is null).  STORED_Z (IC, AMG): z does not exist yet and dinv is not read: the partials of r.r alone ->
// part_out[2 * block + 1]; r.z follows from cg_rz_kernel once z is there.
template <bool STORED_Z>
__global__ __launch_bounds__(dev::kBlock)
void cg_update_kernel(int n, int step, const float* __restrict__ p, const float* __restrict__ q,
                      const float* __restrict__ dinv, float* __restrict__ x, float* __restrict__ r,
                      CgState* __restrict__ state, const double* __restrict__ pq_part, int pq_count,
                      double* __restrict__ part_out) {
    if (state->done) return;
    double pq = 0.0, unused = 0.0;
    solver::fold_partials(pq_part, pq_count, 1, pq, unused);
    if (!(pq > 0.0)) {             // A is not SPD (or p.q is not finite): x stays at the last good iterate
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->breakdown = 1;
            state->done = 1;
        }
        return;
    }
    const float alpha = static_cast<float>(state->rz[step & 1] / pq);
    double rz = 0.0, rr = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * dev::kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * dev::kBlock) {
        const float pi = p[i];
        const float qi = q[i];
        x[i] = __builtin_fmaf(alpha, pi, x[i]);
        const float ri = __builtin_fmaf(-alpha, qi, r[i]);
        r[i] = ri;
        if constexpr (!STORED_Z) {
            const float zi = dinv ? __fmul_rn(ri, dinv[i]) : ri;
            rz += solver::prod64(ri, zi);
        }
        rr += solver::prod64(ri, ri);
    }
    if constexpr (STORED_Z) {
        dev::block_sum2(rr, unused);
        if (threadIdx.x == 0) part_out[2 * blockIdx.x + 1] = rr;
    } else {
        dev::block_sum2(rz, rr);
        if (threadIdx.x == 0) {
            part_out[2 * blockIdx.x] = rz;
            part_out[2 * blockIdx.x + 1] = rr;
        }
    }
}

// Stored z: block partials of r.z -> part[stride * block] (stride 2 inside the loop, 3 over the init partials).
__global__ __launch_bounds__(dev::kBlock)
void cg_rz_kernel(int n, const float* __restrict__ r, const float* __restrict__ z,
                  const CgState* __restrict__ state, double* __restrict__ part, int stride) {
    if (state->done) return;
    double rz = 0.0, unused = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * dev::kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * dev::kBlock) {
        rz += solver::prod64(r[i], z[i]);
    }
    dev::block_sum2(rz, unused);
    if (threadIdx.x == 0) part[static_cast<long long>(stride) * blockIdx.x] = rz;
}

} // namespace

} // namespace detail
} // namespace spmv

#endif
