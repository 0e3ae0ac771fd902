// bicgstab.hip — device-resident Jacobi-preconditioned BiCGSTAB (include/spmv/bicgstab.h).
//
// Built like cg.hip: alpha, omega, rho and the stop tests live in a device BicgState, every loop kernel returns at
// once when `done` is set, and the host reads a two-deep pinned mirror of the state so that it enqueues step k+1
// before it looks at the outcome of step k.  Per step on the direct engine, five launches:
//   bicg_spmv_dot<LANES>   v = A p^ (vector CSR) and the block partials of r^.v
//   bicg_s_kernel          every workgroup folds the r^.v partials (same order => same alpha everywhere), then
//                          s = r - alpha v (in place of r), s^ = s * dinv, and the block partials of s.s
//   bicg_spmv_dot<LANES>   t = A s^ and the block partials of t.s and t.t
//   bicg_update_kernel     folds s.s, t.s, t.t: the half-step stop or omega; x += alpha p^ + omega s^, r = s - omega t,
//                          and the block partials of r.r and r^.r
//   bicg_direction_kernel  folds those: the stop and RHO tests, commits the step (workgroup 0); beta, p and p^
// On the tiled engine tiled_spmv(plan, p^, v) / tiled_spmv(plan, s^, t) and bicg_dot_kernel replace the fused SpMVs.
// A step's outcome is committed to the state only by the last kernel that does work in it, so no workgroup of a
// kernel that still has vector work to do can see `done` early.  Dot products accumulate fp64 products of the fp32
// entries; no float atomics anywhere.
//
// bicgstab_solve_lu is the same loop with M = L U given as a factor matrix: the step kernels run as with NONE
// (dinv == nullptr, no p^ / s^ outputs) and p^ = U^-1 (L^-1 p), s^ = U^-1 (L^-1 s) are two launch_sptrsv sequences each
// (TriangularPair::apply) into the stored p^ / s^ buffers, s^ after bicg_s_kernel and p^ after bicg_direction_kernel.
// The solve kernels do not read `done`: after it they still write p^ / s^, which nothing reads any more.
//
// The host side is built from solver_common.h's parts (Workspace and its mirror, TriangularPair, TiledEngine,
// diag_kernel); what is here is this solver's checks, its workspace layout, its launches and its result.
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"
#include "tiled.h"
#include "spmv/bicgstab.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

// How a step ended at its half step (bicg_update_kernel decides, bicg_direction_kernel commits).
enum HalfStop { kNoHalfStop = 0, kHalfConverged = 1, kOmegaAfterHalfStep = 2, kOmegaBeforeHalfStep = 3 };

// Lives in device memory; every loop kernel reads `done` first.  rho is double-buffered by step parity: step k
// reads rho[k & 1] and its direction kernel writes rho[(k + 1) & 1], so no workgroup reads a slot another is writing.
struct BicgState {
    double rho[2];            // r^.r of the current residual
    double bnorm;             // ||b||_2
    double threshold;         // tolerance * ||b||_2
    float  alpha;             // this step's alpha (bicg_s_kernel, workgroup 0)
    float  omega;             // this step's omega (bicg_update_kernel, workgroup 0)
    float  relative_residual; // ||r||_2 / ||b||_2 of the last committed step
    float  half_residual;     // ||s||_2 / ||b||_2 of this step
    int    iterations;        // committed steps
    int    converged;
    int    breakdown;         // BiCGStabResult::Breakdown
    int    done;              // steps after this are no-ops
    int    zero_b;            // ||b|| == 0: the host writes x = 0
    int    bad_diagonal;      // JACOBI: some row's diagonal is missing, zero or not finite
    int    half_stop;         // HalfStop of this step
    int    reserved;
};

__device__ __forceinline__ bool usable(double v) { return v != 0.0 && isfinite(v); }

// r0 = b - A x0, r^ = p0 = r0, p^0 = r0 * dinv (JACOBI), and the block partials of r.r and b.b -> part[2 * block].
template <int LANES>
__global__ __launch_bounds__(kBlock)
void bicg_init_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                      const float* __restrict__ vals, const float* __restrict__ b, const float* __restrict__ x,
                      const float* __restrict__ dinv, float* __restrict__ r, float* __restrict__ rhat,
                      float* __restrict__ p, float* __restrict__ phat, double* __restrict__ part) {
    double rr = 0.0, bb = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        const float bi = b[row];
        const float ri = __fsub_rn(bi, acc);
        r[row] = ri;
        rhat[row] = ri;
        p[row] = ri;
        if (dinv) phat[row] = __fmul_rn(ri, dinv[row]);
        rr += prod64(ri, ri);
        bb += prod64(bi, bi);
    });
    block_sum2(rr, bb);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = rr;
        part[2 * blockIdx.x + 1] = bb;
    }
}

// One workgroup: folds the init partials and sets up the state (rho[0] = r^.r0 = r0.r0, ||b||, the threshold, the
// step-0 outcome).
__global__ __launch_bounds__(kBlock)
void bicg_start_kernel(const double* __restrict__ part, int count, float tolerance, BicgState* __restrict__ state) {
    double rr = 0.0, bb = 0.0;
    fold_partials(part, count, 2, rr, bb);
    if (threadIdx.x != 0) return;
    const double bnorm = sqrt(bb);
    const double res = sqrt(rr);
    state->rho[0] = rr;
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
    } else if (!usable(rr)) {
        state->breakdown = BiCGStabResult::RHO;
        state->done = 1;
    }
}

// y = A w and the block partials of a.y (and y.y when with_yy) -> part[block] (part[2 * block], part[2 * block + 1]).
// a_i is the row's own entry: y is not read back.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void bicg_spmv_dot(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                   const float* __restrict__ vals, const float* __restrict__ w, float* __restrict__ y,
                   const float* __restrict__ a, int with_yy, const BicgState* __restrict__ state,
                   double* __restrict__ part) {
    if (state->done) return;
    double ay = 0.0, yy = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, w, [&](long long row, float acc) {
        y[row] = acc;
        ay += prod64(a[row], acc);
        yy += prod64(acc, acc);
    });
    block_sum2(ay, yy);
    if (threadIdx.x == 0) {
        if (with_yy) {
            part[2 * blockIdx.x] = ay;
            part[2 * blockIdx.x + 1] = yy;
        } else {
            part[blockIdx.x] = ay;
        }
    }
}

// Block partials of a.y (and y.y when with_yy), laid out as bicg_spmv_dot's (tiled engine: y came from tiled_spmv).
__global__ __launch_bounds__(kBlock)
void bicg_dot_kernel(int n, const float* __restrict__ a, const float* __restrict__ y, int with_yy,
                     const BicgState* __restrict__ state, double* __restrict__ part) {
    if (state->done) return;
    double ay = 0.0, yy = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float yi = y[i];
        ay += prod64(a[i], yi);
        yy += prod64(yi, yi);
    }
    block_sum2(ay, yy);
    if (threadIdx.x == 0) {
        if (with_yy) {
            part[2 * blockIdx.x] = ay;
            part[2 * blockIdx.x + 1] = yy;
        } else {
            part[blockIdx.x] = ay;
        }
    }
}

// alpha = rho_k / r^.v (ALPHA breakdown if r^.v is 0 or not finite: nothing is written but the state);
// s = fmaf(-alpha, v, r) over r; s^ = s * dinv (JACOBI); partials of s.s -> ss_part[block].
__global__ __launch_bounds__(kBlock)
void bicg_s_kernel(int n, int step, const float* __restrict__ v, const float* __restrict__ dinv, float* __restrict__ r,
                   float* __restrict__ shat, BicgState* __restrict__ state, const double* __restrict__ rv_part,
                   int rv_count, double* __restrict__ ss_part) {
    if (state->done) return;
    double rv = 0.0, unused = 0.0;
    fold_partials(rv_part, rv_count, 1, rv, unused);
    if (!usable(rv)) {            // no workgroup writes a vector: x stays x_k
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->breakdown = BiCGStabResult::ALPHA;
            state->done = 1;
        }
        return;
    }
    const float alpha = static_cast<float>(state->rho[step & 1] / rv);
    if (blockIdx.x == 0 && threadIdx.x == 0) state->alpha = alpha;
    double ss = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float si = __builtin_fmaf(-alpha, v[i], r[i]);
        r[i] = si;
        if (dinv) shat[i] = __fmul_rn(si, dinv[i]);
        ss += prod64(si, si);
    }
    block_sum2(ss, unused);
    if (threadIdx.x == 0) ss_part[blockIdx.x] = ss;
}

// The half-step test on ||s||, else omega = t.s / t.t (OMEGA breakdown if 0 or not finite); x and r; partials of
// r.r and r^.r -> rr_part[2 * block].  A half stop is left in the state for bicg_direction_kernel to commit.
// With NONE, shat is s (the r buffer) and phat is p: no __restrict__ on those.
__global__ __launch_bounds__(kBlock)
void bicg_update_kernel(int n, const float* phat, const float* shat, const float* __restrict__ t,
                        const float* __restrict__ rhat, float* __restrict__ x, float* r, BicgState* __restrict__ state,
                        const double* __restrict__ ss_part, int ss_count, const double* __restrict__ ts_part,
                        int ts_count, double* __restrict__ rr_part) {
    if (state->done) return;
    double ss = 0.0, ts = 0.0, tt = 0.0, unused = 0.0;
    fold_partials(ss_part, ss_count, 1, ss, unused);
    fold_partials(ts_part, ts_count, 2, ts, tt);
    const float alpha = state->alpha;
    const double sres = sqrt(ss);
    int stop = kNoHalfStop;
    float omega = 0.0f;
    if (sres <= state->threshold) {
        stop = kHalfConverged;
    } else {
        omega = static_cast<float>(ts / tt);
        if (!usable(omega)) stop = isfinite(sres) ? kOmegaAfterHalfStep : kOmegaBeforeHalfStep;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->omega = omega;
        state->half_stop = stop;
        state->half_residual = static_cast<float>(sres / state->bnorm);
    }
    if (stop == kOmegaBeforeHalfStep) return;
    if (stop != kNoHalfStop) {    // x_k + alpha p^: the half step whose residual is s
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            x[i] = __builtin_fmaf(alpha, phat[i], x[i]);
        }
        return;
    }
    double rr = 0.0, rho = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        x[i] = __builtin_fmaf(omega, shat[i], __builtin_fmaf(alpha, phat[i], x[i]));
        const float ri = __builtin_fmaf(-omega, t[i], r[i]);
        r[i] = ri;
        rr += prod64(ri, ri);
        rho += prod64(rhat[i], ri);
    }
    block_sum2(rr, rho);
    if (threadIdx.x == 0) {
        rr_part[2 * blockIdx.x] = rr;
        rr_part[2 * blockIdx.x + 1] = rho;
    }
}

// Commits the step (workgroup 0): a half stop, or the stop and RHO tests on r.r and r^.r.  Otherwise
// beta = (rho_k+1 / rho_k) (alpha / omega), p = fmaf(beta, fmaf(-omega, v, p), r), p^ = p * dinv (JACOBI).
__global__ __launch_bounds__(kBlock)
void bicg_direction_kernel(int n, int step, const float* __restrict__ v, const float* __restrict__ r,
                           const float* __restrict__ dinv, float* __restrict__ p, float* __restrict__ phat,
                           BicgState* __restrict__ state, const double* __restrict__ rr_part, int rr_count) {
    if (state->done) return;
    const int stop = state->half_stop;
    if (stop != kNoHalfStop) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->iterations = stop == kOmegaBeforeHalfStep ? step : step + 1;
            state->relative_residual = state->half_residual;
            if (stop == kHalfConverged) state->converged = 1;
            else state->breakdown = BiCGStabResult::OMEGA;
            state->done = 1;
        }
        return;
    }
    double rr = 0.0, rho = 0.0;
    fold_partials(rr_part, rr_count, 2, rr, rho);
    const double res = sqrt(rr);
    const bool converged = res <= state->threshold;
    const bool breakdown = !converged && !usable(rho);
    const double rho_old = state->rho[step & 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->iterations = step + 1;
        state->relative_residual = static_cast<float>(res / state->bnorm);
        state->rho[(step + 1) & 1] = rho;
        if (converged) state->converged = 1;
        if (breakdown) state->breakdown = BiCGStabResult::RHO;
        if (converged || breakdown) state->done = 1;
    }
    if (converged || breakdown) return;
    const float alpha = state->alpha;
    const float omega = state->omega;
    const float beta = static_cast<float>((rho / rho_old) * (static_cast<double>(alpha) / static_cast<double>(omega)));
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float pi = __builtin_fmaf(beta, __builtin_fmaf(-omega, v[i], p[i]), r[i]);
        p[i] = pi;
        if (dinv) phat[i] = __fmul_rn(pi, dinv[i]);
    }
}

hipError_t init(int lanes, const CSRMatrix* A, const float* b, const float* x, const float* dinv, float* r,
                float* rhat, float* p, float* phat, double* part, int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        bicg_init_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                    A->d_col_indices, A->d_values, b, x, dinv, r,
                                                                    rhat, p, phat, part);
        return hipGetLastError();
    });
}

hipError_t spmv_dot(int lanes, const CSRMatrix* A, const float* w, float* y, const float* a, int with_yy,
                    const BicgState* state, double* part, int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        bicg_spmv_dot<decltype(L)::value><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                 A->d_col_indices, A->d_values, w, y, a, with_yy,
                                                                 state, part);
        return hipGetLastError();
    });
}

// bicgstab_solve (with_lu false: LU is not looked at, cfg.preconditioner picks NONE or JACOBI) and bicgstab_solve_lu
// (with_lu true: M = L U from LU, cfg.preconditioner is not read).
BiCGStabResult solve(const CSRMatrix* A, const CSRMatrix* LU, bool with_lu, const float* d_b, float* d_x,
                     const BiCGStabConfig* config) {
    BiCGStabResult result;
    const auto fail = [&result](SpMVError e) {
        result.error_code = code(e);
        return result;
    };
    if (!A || !d_b || !d_x || (with_lu && !LU)) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return fail(SpMVError::INVALID_DIMENSION);
    if (with_lu && (LU->num_rows != LU->num_cols || LU->num_rows != A->num_rows)) {
        return fail(SpMVError::INVALID_DIMENSION);
    }
    if (A->num_rows == 0) {
        result.converged = 1;
        return result;
    }
    if (!device_arrays(A) || (with_lu && !device_arrays(LU))) return fail(SpMVError::INVALID_FORMAT);
    const BiCGStabConfig defaults;
    const BiCGStabConfig& cfg = config ? *config : defaults;
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 ||
        (!with_lu && cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI) ||
        cfg.engine < -1 || cfg.engine > 1) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const int n = A->num_rows;
    if (ranges_overlap(d_b, d_x, n)) return fail(SpMVError::INVALID_ARGUMENT);

    const TraceRange range(with_lu ? "spmv:bicgstab_solve_lu" : "spmv:bicgstab_solve");
    hipStream_t stream = current_stream();
    const bool jacobi = !with_lu && cfg.preconditioner == CGConfig::JACOBI;
    const bool stored = jacobi || with_lu;         // p^ and s^ are buffers of their own

    TriangularPair lu;              // M = L U: L's diagonal is the implied 1
    if (with_lu) {
        const int status = lu.build(LU, 1, stream);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }
    TiledEngine engine(A, cfg.engine, stream);

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const size_t dot_count = static_cast<size_t>(std::max(row_grid, vgrid));
    const size_t rv_count = dot_count;
    const size_t ss_count = static_cast<size_t>(vgrid);
    const size_t ts_count = 2 * dot_count;
    const size_t rr_count = 2 * static_cast<size_t>(vgrid);
    const size_t init_count = 2 * static_cast<size_t>(row_grid);

    // r (s in place), r^, p, v, t; with JACOBI or an LU also p^ and s^, with JACOBI dinv (with NONE p^ is p and s^ is s)
    Workspace<BicgState> ws;
    const size_t len = static_cast<size_t>(n);
    if (!ws.allocate((jacobi ? 8 : stored ? 7 : 5) * len, rv_count + ss_count + ts_count + rr_count + init_count)) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    float* r = ws.vec;
    float* rhat = ws.vec + len;
    float* p = ws.vec + 2 * len;
    float* v = ws.vec + 3 * len;
    float* t = ws.vec + 4 * len;
    float* phat = stored ? ws.vec + 5 * len : p;
    float* shat = stored ? ws.vec + 6 * len : r;
    float* dinv = jacobi ? ws.vec + 7 * len : nullptr;
    double* rv_part = ws.part;
    double* ss_part = rv_part + rv_count;
    double* ts_part = ss_part + ss_count;
    double* rr_part = ts_part + ts_count;
    double* init_part = rr_part + rr_count;

    // setup: diagonal (JACOBI; of LU, only its check), r0 / r^ / p0 / p^0 and their dots, the state; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(BicgState), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (with_lu) ok = ok && launch_diag<DiagRule::NONZERO_FINITE>(LU, nullptr, bad, stream) == hipSuccess;
    if (jacobi) ok = ok && launch_diag<DiagRule::NONZERO_FINITE>(A, dinv, bad, stream) == hipSuccess;
    float* phat_out = jacobi ? phat : nullptr;     // the kernels write p^ / s^ only with JACOBI
    float* shat_out = jacobi ? shat : nullptr;
    ok = ok && init(lanes, A, d_b, d_x, dinv, r, rhat, p, phat_out, init_part, row_grid, stream) == hipSuccess;
    if (with_lu) ok = ok && lu.apply(p, phat, stream);
    if (ok) {
        bicg_start_kernel<<<1, kBlock, 0, stream>>>(init_part, row_grid, cfg.tolerance, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (ws.pinned[0].bad_diagonal) return fail(SpMVError::INVALID_ARGUMENT);
    if (ws.pinned[0].zero_b) {
        if (!zero_solution(d_x, len, stream)) return fail(SpMVError::KERNEL_LAUNCH);
        result.converged = 1;
        return result;
    }

    // y = A w plus the partials of a.y (and y.y): tiled_spmv + bicg_dot_kernel while a plan is held, else the fused
    // direct kernel.  `count` receives the number of partials written.
    const auto spmv_and_dot = [&](const float* w, float* y, const float* a, int with_yy, double* part,
                                  int& count) -> bool {
        const TiledEngine::Spmv spmv = engine.spmv(w, y, stream);
        if (spmv == TiledEngine::Spmv::FAILED) return false;
        if (spmv == TiledEngine::Spmv::TILED) {
            bicg_dot_kernel<<<vgrid, kBlock, 0, stream>>>(n, a, y, with_yy, ws.state, part);
            count = vgrid;
            return hipGetLastError() == hipSuccess;
        }
        count = row_grid;
        return spmv_dot(lanes, A, w, y, a, with_yy, ws.state, part, row_grid, stream) == hipSuccess;
    };

    if (!ws.pinned[0].done) {
        EventPair& ev = thread_events();
        ok = hipEventRecord(ev.start, stream) == hipSuccess;
        for (int iter = 0; ok && iter < cfg.max_iterations; ++iter) {
            if (!engine.build_if_due(iter, ws, stream, ok)) break;
            const TraceRange step_range("spmv:bicgstab_step");
            int rv_parts = 0, ts_parts = 0;
            ok = spmv_and_dot(phat, v, rhat, 0, rv_part, rv_parts);
            if (ok) {
                bicg_s_kernel<<<vgrid, kBlock, 0, stream>>>(n, iter, v, dinv, r, shat_out, ws.state, rv_part, rv_parts,
                                                            ss_part);
                ok = hipGetLastError() == hipSuccess;
            }
            if (with_lu) ok = ok && lu.apply(r, shat, stream);
            ok = ok && spmv_and_dot(shat, t, r, 1, ts_part, ts_parts);
            if (ok) {
                bicg_update_kernel<<<vgrid, kBlock, 0, stream>>>(n, phat, shat, t, rhat, d_x, r, ws.state, ss_part,
                                                                 vgrid, ts_part, ts_parts, rr_part);
                bicg_direction_kernel<<<vgrid, kBlock, 0, stream>>>(n, iter, v, r, dinv, p, phat_out, ws.state, rr_part,
                                                                    vgrid);
                ok = hipGetLastError() == hipSuccess && (!with_lu || lu.apply(p, phat, stream))
                  && ws.publish(iter, sizeof(BicgState), stream);
            }
            if (ok && iter >= 1) {
                const BicgState* seen = ws.wait_previous(iter);
                ok = seen != nullptr;
                if (ok && seen->done) break;
            }
        }
        if (!ws.finish_timed(ok, ev, stream, &result.elapsed_ms)) return fail(SpMVError::KERNEL_LAUNCH);
    }
    const BicgState& final_state = ws.pinned[0];
    result.iterations = final_state.iterations;
    result.relative_residual = final_state.relative_residual;
    result.converged = final_state.converged;
    result.breakdown = final_state.breakdown;
    return result;
}

} // namespace
} // namespace detail

BiCGStabResult bicgstab_solve(const CSRMatrix* A, const float* d_b, float* d_x, const BiCGStabConfig* config) {
    return detail::solve(A, nullptr, false, d_b, d_x, config);
}

BiCGStabResult bicgstab_solve_lu(const CSRMatrix* A, const CSRMatrix* LU, const float* d_b, float* d_x,
                                 const BiCGStabConfig* config) {
    return detail::solve(A, LU, true, d_b, d_x, config);
}

} // namespace spmv
