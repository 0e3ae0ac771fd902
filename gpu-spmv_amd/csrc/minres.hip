// minres.hip — device-resident preconditioned MINRES for symmetric indefinite systems (include/spmv/minres.h,
// DESIGN.md §4.33).
//
// Built like cg.hip: the Lanczos and rotation scalars live in a device MinresState, every loop kernel returns at once
// when `done` is set, and the host reads a two-deep pinned mirror of the state so that it enqueues step k+1 before it
// looks at the outcome of step k.  Per step on the direct engine, three launches whatever the matrix:
//   minres_spmv_dot<LANES>     y = A v - sigma v - (beta / oldb) r1 (vector CSR), written over r1, and the block
//                              partials of v.y
//   minres_lanczos_kernel      every workgroup folds the v.y partials (same order => same alpha everywhere), then
//                              y -= (alpha / beta) r2 and, with a diagonal M, the block partials of y.(dinv y)
//   minres_update_kernel       every workgroup folds those partials, gets beta and advances the rotation identically;
//                              workgroup 0 commits the state; w_k over w_k-2, x += phi w_k, the next v, the stop test
// On the tiled engine tiled_spmv(plan, v, q) and minres_vec_dot_kernel (the vector part of the first launch, from q)
// replace the first launch.
//
// minres_solve_ic is the same loop with M = L L^T given as a factor matrix.  z = M^-1 y is a stored vector there:
// between the second and the third launch come TriangularPair::apply(y -> z) and minres_dot_kernel (the partials of
// y.z); the solves do not read `done`: after it y no longer changes and they rewrite the same z.
//
// The rotation state is double-buffered by step parity: step k reads rot[k & 1] and its update kernel writes
// rot[(k + 1) & 1], so no workgroup reads a slot another is writing.  r1, r2 and y share two buffers that swap roles
// by step parity on the host: y is written over r1 by the one kernel that reads r1.  w_k-1 and w_k-2 swap the same way.
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"
#include "tiled.h"
#include "spmv/minres.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

struct MinresRotation {
    double beta;              // beta_k+1 = sqrt(r2.M^-1 r2) of the current r2
    double oldb;              // beta_k
    double dbar, epsln, phibar, cs, sn;
};

// Lives in device memory; every loop kernel reads `done` first.
struct MinresState {
    MinresRotation rot[2];    // by step parity
    double alpha;             // v.y of the step in flight: written by the Lanczos kernel, read by the update kernel
    double bnorm;             // ||b||_2
    double bmnorm;            // sqrt(b.M^-1 b)
    double threshold;         // tolerance * sqrt(b.M^-1 b)
    float  relative_residual; // phibar / sqrt(b.M^-1 b) of the last committed step
    int    iterations;        // committed steps
    int    converged;
    int    breakdown;         // MinresResult::Breakdown
    int    done;              // steps after this are no-ops
    int    zero_b;            // ||b|| == 0: the host writes x = 0
    int    bad_diagonal;      // JACOBI: a diagonal is missing, equal to the shift or not finite; IC: F's rule
    int    lanczos_step;      // step + 1 of the last step whose Lanczos kernel went through: what the update kernel waits on
};

// JACOBI's M = |diag(A - sigma I)|: d = fp32(the fp32 sum of row i's stored (i,i) entries in storage order - sigma),
// dinv[i] = 1 / |d|, or 0 for a row that has no stored diagonal or whose d is 0 or not finite; *bad_flag = 1 if any
// row is rejected.  diag_kernel's walk (solver_common.h) with the shift and the absolute value; one thread per row:
// setup only.
__global__ __launch_bounds__(kBlock)
void minres_diag_kernel(int n, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                        const float* __restrict__ vals, float shift, float* __restrict__ dinv,
                        int* __restrict__ bad_flag) {
    int bad = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float d = 0.0f;
        int found = 0;
        for (int j = row_ptrs[i]; j < row_ptrs[i + 1]; ++j) {
            if (cols[j] == i) {
                d = __fadd_rn(d, vals[j]);
                found = 1;
            }
        }
        d = fabsf(__fsub_rn(d, shift));
        const bool ok = found && d != 0.0f && isfinite(d);
        dinv[i] = ok ? __fdiv_rn(1.0f, d) : 0.0f;
        bad |= !ok;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *bad_flag = 1;
}

// r0 = b - (A - sigma I) x0 -> r, and the block partials -> part[3 * block]: r0.(dinv r0), b.(dinv b), b.b (dinv
// null: M = I).  STORED_Z: M^-1 is not a diagonal, the first two slots are filled by minres_dot_kernel later.
template <int LANES, bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void minres_init_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                        const float* __restrict__ vals, float shift, const float* __restrict__ b,
                        const float* __restrict__ x, const float* __restrict__ dinv, float* __restrict__ r,
                        double* __restrict__ part) {
    double rz = 0.0, bz = 0.0, bb = 0.0, unused = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        const float bi = b[row];
        const float ri = __fsub_rn(bi, __builtin_fmaf(-shift, x[row], acc));
        r[row] = ri;
        if constexpr (!STORED_Z) {
            const float di = dinv ? dinv[row] : 1.0f;
            rz += prod64(ri, dinv ? __fmul_rn(ri, di) : ri);
            bz += prod64(bi, dinv ? __fmul_rn(bi, di) : bi);
        }
        bb += prod64(bi, bi);
    });
    if constexpr (!STORED_Z) {
        block_sum2(rz, bz);
        if (threadIdx.x == 0) {
            part[3 * blockIdx.x] = rz;
            part[3 * blockIdx.x + 1] = bz;
        }
    }
    block_sum2(bb, unused);
    if (threadIdx.x == 0) part[3 * blockIdx.x + 2] = bb;
}

// Block partials of a.c -> part[stride * block]: the stored-z dot products (setup: stride 3 over the init partials,
// state null; the loop: y.z, stride 1).
__global__ __launch_bounds__(kBlock)
void minres_dot_kernel(int n, const float* __restrict__ a, const float* __restrict__ c,
                       const MinresState* __restrict__ state, double* __restrict__ part, int stride) {
    if (state && state->done) return;
    double ac = 0.0, unused = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        ac += prod64(a[i], c[i]);
    }
    block_sum2(ac, unused);
    if (threadIdx.x == 0) part[static_cast<long long>(stride) * blockIdx.x] = ac;
}

// One workgroup: folds the init partials and sets up the state (rot[0], the norms, the threshold, step-0 outcome).
__global__ __launch_bounds__(kBlock)
void minres_start_kernel(const double* __restrict__ part, int count, float tolerance,
                         MinresState* __restrict__ state) {
    double rz = 0.0, bz = 0.0, bb = 0.0, unused = 0.0;
    fold_partials(part, count, 3, rz, bz);
    fold_partials(part + 2, count, 3, bb, unused, false);    // part[3 * count] is past the end: b.b alone
    if (threadIdx.x != 0) return;
    const double bnorm = sqrt(bb);
    const double bmnorm = sqrt(bz);
    const double beta1 = sqrt(rz);
    MinresRotation& rot = state->rot[0];
    rot.beta = beta1;
    rot.oldb = 0.0;
    rot.dbar = 0.0;
    rot.epsln = 0.0;
    rot.phibar = beta1;
    rot.cs = -1.0;
    rot.sn = 0.0;
    state->bnorm = bnorm;
    state->bmnorm = bmnorm;
    state->threshold = static_cast<double>(tolerance) * bmnorm;
    state->iterations = 0;
    if (bb == 0.0) {
        state->zero_b = 1;
        state->relative_residual = 0.0f;
        state->converged = 1;
        state->done = 1;
        return;
    }
    state->relative_residual = static_cast<float>(beta1 / bmnorm);
    if (!isfinite(rz) || !isfinite(bz) || !isfinite(bb)) {
        state->breakdown = MinresResult::NOT_FINITE;
        state->done = 1;
    } else if (rz < 0.0 || !(bz > 0.0)) {                     // b != 0 and b.M^-1 b <= 0: M is not positive definite
        state->breakdown = MinresResult::PRECONDITIONER;
        state->done = 1;
    } else if (beta1 <= state->threshold) {                   // beta_1 == 0 included
        state->converged = 1;
        state->done = 1;
    }
}

// The first Lanczos vector: v = (M^-1 r0) / fp32(beta_1).  zr is r0 and M^-1 r0 = r0 * dinv (r0 where dinv is null),
// or with STORED_Z it is z itself.
template <bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void minres_first_v_kernel(int n, const float* __restrict__ zr, const float* __restrict__ dinv,
                           float* __restrict__ v, const MinresState* __restrict__ state) {
    if (state->done) return;
    const float bt = static_cast<float>(state->rot[0].beta);
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float zi = zr[i];
        if constexpr (!STORED_Z) zi = dinv ? __fmul_rn(zi, dinv[i]) : zi;
        v[i] = __fdiv_rn(zi, bt);
    }
}

// c1 = fp32(beta / oldb) of step `step` (0-based); not read at step 0, where r1 does not exist
__device__ __forceinline__ float three_term_coefficient(const MinresState* state, int step) {
    const MinresRotation& rot = state->rot[step & 1];
    return step > 0 ? static_cast<float>(rot.beta / rot.oldb) : 0.0f;
}

// y = A v - sigma v - c1 r1, written over r1 (its last use), and the block partials of v.y -> part[block].  v_i is
// the row's own entry.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void minres_spmv_dot(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                     const float* __restrict__ vals, float shift, int step, const float* __restrict__ v,
                     float* __restrict__ y, const MinresState* __restrict__ state, double* __restrict__ part) {
    if (state->done) return;
    const float c1 = three_term_coefficient(state, step);
    double vy = 0.0, unused = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, v, [&](long long row, float acc) {
        const float vi = v[row];
        float yi = __builtin_fmaf(-shift, vi, acc);
        if (step > 0) yi = __builtin_fmaf(-c1, y[row], yi);
        y[row] = yi;
        vy += prod64(vi, yi);
    });
    block_sum2(vy, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = vy;
}

// The same from q = A v (tiled engine: q came from tiled_spmv).
__global__ __launch_bounds__(kBlock)
void minres_vec_dot_kernel(int n, float shift, int step, const float* __restrict__ v, const float* __restrict__ q,
                           float* __restrict__ y, const MinresState* __restrict__ state,
                           double* __restrict__ part) {
    if (state->done) return;
    const float c1 = three_term_coefficient(state, step);
    double vy = 0.0, unused = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float vi = v[i];
        float yi = __builtin_fmaf(-shift, vi, q[i]);
        if (step > 0) yi = __builtin_fmaf(-c1, y[i], yi);
        y[i] = yi;
        vy += prod64(vi, yi);
    }
    block_sum2(vy, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = vy;
}

// alpha = v.y; y -= (alpha / beta) r2; the partials of y.(dinv y) (y.y where dinv is null) -> part_out[block].
// STORED_Z: z does not exist yet and dinv is not read: no partials; y.z follows from minres_dot_kernel.
template <bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void minres_lanczos_kernel(int n, int step, const float* __restrict__ r2, const float* __restrict__ dinv,
                           float* __restrict__ y, MinresState* __restrict__ state,
                           const double* __restrict__ vy_part, int vy_count, double* __restrict__ part_out) {
    if (state->done) return;
    double alpha = 0.0, unused = 0.0;
    fold_partials(vy_part, vy_count, 1, alpha, unused);
    if (!isfinite(alpha)) {             // x stays at the last committed iterate
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->breakdown = MinresResult::NOT_FINITE;
            state->done = 1;
        }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->alpha = alpha;
        state->lanczos_step = step + 1;
    }
    const float c2 = static_cast<float>(alpha / state->rot[step & 1].beta);
    double yz = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float yi = __builtin_fmaf(-c2, r2[i], y[i]);
        y[i] = yi;
        if constexpr (!STORED_Z) yz += prod64(yi, dinv ? __fmul_rn(yi, dinv[i]) : yi);
    }
    if constexpr (!STORED_Z) {
        block_sum2(yz, unused);
        if (threadIdx.x == 0) part_out[blockIdx.x] = yz;
    }
}

// beta = sqrt(y.z), the rotation, the stop test; w_k over w_k-2, x += phi w_k, the next v = z / beta.  Workgroup 0
// commits the step to the state.  zy is y and z = y * dinv (y where dinv is null), or with STORED_Z it is z itself and
// dinv is not read.  The only loop kernel that does not read `done` (see its first line).
template <bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void minres_update_kernel(int n, int step, const float* __restrict__ zy, const float* __restrict__ dinv,
                          float* __restrict__ v, const float* __restrict__ w_prev, float* __restrict__ w,
                          float* __restrict__ x, MinresState* __restrict__ state, const double* __restrict__ part,
                          int count) {
    // Not `done`: workgroup 0 sets it below when the step converges, while the others still have their part of w, x
    // to write.  The Lanczos kernel of this step read `done` and has (or has not) left its mark; nothing here writes it.
    if (state->lanczos_step != step + 1) return;
    double yz = 0.0, unused = 0.0;
    fold_partials(part, count, 1, yz, unused);
    const MinresRotation old = state->rot[step & 1];
    const double alpha = state->alpha;
    const double beta = sqrt(yz);
    const double oldeps = old.epsln;
    const double delta = old.cs * old.dbar + old.sn * alpha;
    const double gbar = old.sn * old.dbar - old.cs * alpha;
    const double gamma = sqrt(gbar * gbar + beta * beta);
    int breakdown = MinresResult::NONE;
    if (!isfinite(yz)) breakdown = MinresResult::NOT_FINITE;
    else if (yz < 0.0) breakdown = MinresResult::PRECONDITIONER;
    else if (!isfinite(gamma)) breakdown = MinresResult::NOT_FINITE;
    else if (gamma == 0.0) breakdown = MinresResult::SINGULAR;
    if (breakdown != MinresResult::NONE) {          // nothing of this step is committed
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->breakdown = breakdown;
            state->done = 1;
        }
        return;
    }
    const double cs = gbar / gamma;
    const double sn = beta / gamma;
    const double phi = cs * old.phibar;
    const double phibar = sn * old.phibar;
    // |phibar| : sn >= 0 and phibar_0 = beta_1 >= 0, so phibar >= 0 already
    const bool converged = phibar <= state->threshold || beta == 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        MinresRotation& next = state->rot[(step + 1) & 1];
        next.beta = beta;
        next.oldb = old.beta;
        next.dbar = -old.cs * beta;
        next.epsln = old.sn * beta;
        next.phibar = phibar;
        next.cs = cs;
        next.sn = sn;
        state->iterations = step + 1;
        state->relative_residual = static_cast<float>(phibar / state->bmnorm);
        if (converged) {
            state->converged = 1;
            state->done = 1;
        }
    }
    const float oe = static_cast<float>(oldeps);
    const float de = static_cast<float>(delta);
    const float g = static_cast<float>(gamma);
    const float ph = static_cast<float>(phi);
    const float bt = static_cast<float>(beta);
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float wi = __fdiv_rn(__builtin_fmaf(-de, w_prev[i], __builtin_fmaf(-oe, w[i], v[i])), g);
        w[i] = wi;
        x[i] = __builtin_fmaf(ph, wi, x[i]);
        if (!converged) {
            float zi = zy[i];
            if constexpr (!STORED_Z) zi = dinv ? __fmul_rn(zi, dinv[i]) : zi;
            v[i] = __fdiv_rn(zi, bt);
        }
    }
}

// r = b - (A - sigma I) x is not stored: the block partials of r.r -> part[block] (after the loop, once).
template <int LANES>
__global__ __launch_bounds__(kBlock)
void minres_residual_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                            const float* __restrict__ vals, float shift, const float* __restrict__ b,
                            const float* __restrict__ x, double* __restrict__ part) {
    double rr = 0.0, unused = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        const float ri = __fsub_rn(b[row], __builtin_fmaf(-shift, x[row], acc));
        rr += prod64(ri, ri);
    });
    block_sum2(rr, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = rr;
}

template <bool STORED_Z>
hipError_t init(int lanes, const CSRMatrix* A, float shift, const float* b, const float* x, const float* dinv,
                float* r, double* part, int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        minres_init_kernel<decltype(L)::value, STORED_Z><<<grid, kBlock, 0, s>>>(
            A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, shift, b, x, dinv, r, part);
        return hipGetLastError();
    });
}

hipError_t spmv_dot(int lanes, const CSRMatrix* A, float shift, int step, const float* v, float* y,
                    const MinresState* state, double* part, int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        minres_spmv_dot<decltype(L)::value><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                   A->d_col_indices, A->d_values, shift, step, v, y,
                                                                   state, part);
        return hipGetLastError();
    });
}

hipError_t residual(int lanes, const CSRMatrix* A, float shift, const float* b, const float* x, double* part,
                    int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        minres_residual_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(
            A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, shift, b, x, part);
        return hipGetLastError();
    });
}

// F == nullptr: the diagonal inside the step kernels (cfg.preconditioner picks NONE or JACOBI); else a stored z from
// M = L L^T of the factor matrix F, and cfg.preconditioner is not read.
MinresResult solve(const CSRMatrix* A, bool with_ic, const CSRMatrix* F, const float* d_b, float* d_x,
                   const MinresConfig* config) {
    MinresResult result;
    const auto fail = [&result](SpMVError e) {
        result.error_code = code(e);
        return result;
    };
    if (!A || !d_b || !d_x) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return fail(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        result.converged = 1;
        return result;
    }
    if (!device_arrays(A)) return fail(SpMVError::INVALID_FORMAT);
    const MinresConfig defaults;
    const MinresConfig& cfg = config ? *config : defaults;
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 ||
        (!with_ic && cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI) ||
        cfg.engine < -1 || cfg.engine > 1 || !std::isfinite(cfg.shift)) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const int n = A->num_rows;
    if (ranges_overlap(d_b, d_x, n)) return fail(SpMVError::INVALID_ARGUMENT);
    if (with_ic) {
        if (!F) return fail(SpMVError::INVALID_ARGUMENT);
        if (F->num_rows != F->num_cols || F->num_rows != n) return fail(SpMVError::INVALID_DIMENSION);
        if (!device_arrays(F)) return fail(SpMVError::INVALID_FORMAT);
    }

    const TraceRange range(with_ic ? "spmv:minres_solve_ic" : "spmv:minres_solve");
    hipStream_t stream = current_stream();
    const bool jacobi = !with_ic && cfg.preconditioner == CGConfig::JACOBI;
    const float shift = cfg.shift;

    TriangularPair ic;              // M = L L^T: the lower solve reads L's stored diagonal
    if (with_ic) {
        const int status = ic.build(F, 0, stream);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }
    TiledEngine engine(A, cfg.engine, stream);

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const size_t vy_count = static_cast<size_t>(std::max(row_grid, vgrid));
    const size_t yz_count = static_cast<size_t>(vgrid);
    const size_t init_count = 3 * static_cast<size_t>(std::max(row_grid, vgrid));

    // two buffers for r1 / r2 / y, v, two for w_k-1 / w_k-2, q (the tiled engine's A v; setup: M^-1 b), and dinv
    // (JACOBI) or z (IC)
    Workspace<MinresState> ws;
    const size_t len = static_cast<size_t>(n);
    const bool seventh = jacobi || with_ic;
    if (!ws.allocate((seventh ? 7 : 6) * len, vy_count + yz_count + init_count)) return fail(SpMVError::CUDA_MALLOC);
    float* rbuf[2] = {ws.vec, ws.vec + len};
    float* v = ws.vec + 2 * len;
    float* wbuf[2] = {ws.vec + 3 * len, ws.vec + 4 * len};
    float* q = ws.vec + 5 * len;
    float* dinv = jacobi ? ws.vec + 6 * len : nullptr;
    float* z = with_ic ? ws.vec + 6 * len : nullptr;
    double* vy_part = ws.part;
    double* yz_part = ws.part + vy_count;
    double* init_part = yz_part + yz_count;
    std::vector<double> rr_host(static_cast<size_t>(row_grid));

    // setup: the diagonal (JACOBI; of F, only its check), r0 and the dots, the state, the first v; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(MinresState), stream) == hipSuccess &&
              hipMemsetAsync(wbuf[0], 0, 2 * len * sizeof(float), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (with_ic) ok = ok && launch_diag<DiagRule::POSITIVE_FINITE>(F, nullptr, bad, stream) == hipSuccess;
    if (ok && jacobi) {
        minres_diag_kernel<<<vgrid, kBlock, 0, stream>>>(n, A->d_row_ptrs, A->d_col_indices, A->d_values, shift, dinv,
                                                         bad);
        ok = hipGetLastError() == hipSuccess;
    }
    float* r0 = rbuf[0];
    if (with_ic) {
        ok = ok && init<true>(lanes, A, shift, d_b, d_x, nullptr, r0, init_part, row_grid, stream) == hipSuccess;
        // b.M^-1 b through q, which nothing uses yet, then z0 = M^-1 r0 and r0.z0
        ok = ok && ic.apply(d_b, q, stream);
        if (ok) {
            minres_dot_kernel<<<row_grid, kBlock, 0, stream>>>(n, d_b, q, nullptr, init_part + 1, 3);
            ok = hipGetLastError() == hipSuccess && ic.apply(r0, z, stream);
        }
        if (ok) {
            minres_dot_kernel<<<row_grid, kBlock, 0, stream>>>(n, r0, z, nullptr, init_part, 3);
            ok = hipGetLastError() == hipSuccess;
        }
    } else {
        ok = ok && init<false>(lanes, A, shift, d_b, d_x, dinv, r0, init_part, row_grid, stream) == hipSuccess;
    }
    if (ok) {
        minres_start_kernel<<<1, kBlock, 0, stream>>>(init_part, row_grid, cfg.tolerance, ws.state);
        if (with_ic) minres_first_v_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, z, nullptr, v, ws.state);
        else minres_first_v_kernel<false><<<vgrid, kBlock, 0, stream>>>(n, r0, dinv, v, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (ws.pinned[0].bad_diagonal) return fail(SpMVError::INVALID_ARGUMENT);
    if (ws.pinned[0].zero_b) {
        if (!zero_solution(d_x, len, stream)) return fail(SpMVError::KERNEL_LAUNCH);
        result.converged = 1;
        return result;
    }

    EventPair& ev = thread_events();
    ok = hipEventRecord(ev.start, stream) == hipSuccess;
    if (!ws.pinned[0].done) {
        for (int iter = 0; ok && iter < cfg.max_iterations; ++iter) {
            if (!engine.build_if_due(iter, ws, stream, ok)) break;
            const TraceRange step_range("spmv:minres_step");
            float* r2 = rbuf[iter & 1];
            float* y = rbuf[(iter + 1) & 1];          // r1 on entry
            float* w = wbuf[iter & 1];                // w_k-2 on entry
            const float* w_prev = wbuf[(iter + 1) & 1];
            int vy_parts = row_grid;
            const TiledEngine::Spmv spmv = engine.spmv(v, q, stream);
            ok = ok && spmv != TiledEngine::Spmv::FAILED;
            if (spmv == TiledEngine::Spmv::TILED) {
                minres_vec_dot_kernel<<<vgrid, kBlock, 0, stream>>>(n, shift, iter, v, q, y, ws.state, vy_part);
                ok = hipGetLastError() == hipSuccess;
                vy_parts = vgrid;
            } else if (ok) {
                ok = spmv_dot(lanes, A, shift, iter, v, y, ws.state, vy_part, row_grid, stream) == hipSuccess;
            }
            if (ok && with_ic) {
                minres_lanczos_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, r2, nullptr, y, ws.state, vy_part,
                                                                         vy_parts, yz_part);
                ok = hipGetLastError() == hipSuccess && ic.apply(y, z, stream);
                if (ok) {
                    minres_dot_kernel<<<vgrid, kBlock, 0, stream>>>(n, y, z, ws.state, yz_part, 1);
                    minres_update_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, z, nullptr, v, w_prev, w, d_x,
                                                                            ws.state, yz_part, vgrid);
                }
            } else if (ok) {
                minres_lanczos_kernel<false><<<vgrid, kBlock, 0, stream>>>(n, iter, r2, dinv, y, ws.state, vy_part,
                                                                          vy_parts, yz_part);
                minres_update_kernel<false><<<vgrid, kBlock, 0, stream>>>(n, iter, y, dinv, v, w_prev, w, d_x,
                                                                         ws.state, yz_part, vgrid);
            }
            ok = ok && hipGetLastError() == hipSuccess && ws.publish(iter, sizeof(MinresState), stream);
            if (ok && iter >= 1) {
                const MinresState* seen = ws.wait_previous(iter);
                ok = seen != nullptr;
                if (ok && seen->done) break;
            }
        }
    }
    // the 2-norm residual of the x that is returned: the recurrence is in the M^-1-norm
    ok = ok && residual(lanes, A, shift, d_b, d_x, vy_part, row_grid, stream) == hipSuccess &&
         hipMemcpyAsync(rr_host.data(), vy_part, rr_host.size() * sizeof(double), hipMemcpyDeviceToHost, stream) ==
             hipSuccess;
    if (!ws.finish_timed(ok, ev, stream, &result.elapsed_ms)) return fail(SpMVError::KERNEL_LAUNCH);
    const MinresState& final_state = ws.pinned[0];
    double rr = 0.0;
    for (const double part : rr_host) rr += part;     // a fixed order: the same bits from run to run
    result.iterations = final_state.iterations;
    result.relative_residual = final_state.relative_residual;
    result.true_relative_residual = static_cast<float>(std::sqrt(rr) / final_state.bnorm);
    result.converged = final_state.converged;
    result.breakdown = final_state.breakdown;
    return result;
}

} // namespace
} // namespace detail

MinresResult minres_solve(const CSRMatrix* A, const float* d_b, float* d_x, const MinresConfig* config) {
    return detail::solve(A, false, nullptr, d_b, d_x, config);
}

MinresResult minres_solve_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_b, float* d_x,
                             const MinresConfig* config) {
    return detail::solve(A, true, F, d_b, d_x, config);
}

} // namespace spmv
