// cg.hip — device-resident preconditioned conjugate gradient (include/spmv/cg.h).
//
// Built like pagerank.hip: alpha, beta, the residual and the stop test live in a device CgState, every loop
// kernel returns at once when `done` is set, and the host reads a two-deep pinned mirror of the state so that it
// enqueues step k+1 before it looks at the outcome of step k.  Per step on the direct engine, three launches:
//   cg_spmv_dot<LANES>  q = A p (vector CSR) and the block partials of p.q
//   cg_update_kernel<false>     every workgroup folds the p.q partials (same order => same alpha everywhere), then
//                               x += alpha p, r -= alpha q, and the block partials of r.z and r.r (z = r * dinv)
//   cg_direction_kernel<false>  every workgroup folds those partials, gets beta and the stop test, p = z + beta p
// On the tiled engine tiled_spmv(plan, p, q) and cg_dot_kernel (partials of p.q) replace the first launch.
// Dot products accumulate fp64 products of the fp32 entries; no float atomics anywhere.
//
// cg_solve_ic is the same loop with M = L L^T given as a factor matrix.  z is a stored vector
// there, so the second half of a step is
//   cg_update_kernel<true>     the same kernel with STORED_Z: only the block partials of r.r (z does not exist yet)
//   TriangularPair::apply      z = L^-1 r (LOWER NON_UNIT), then z = L^-T z in place (UPPER NON_UNIT); the solves do
//                              not read `done`: after it r no longer changes and they rewrite the same z
//   cg_rz_kernel               the block partials of r.z
//   cg_direction_kernel<true>  the same kernel with z read from memory
// and the SpMV half is the one above, kernel for kernel.
//
// cg_solve_amg is cg_solve_ic's loop with z = one V-cycle of an AMG hierarchy on r (amg_vcycle, amg.hip, DESIGN.md
// §4.16) in place of the two triangular solves; its kernels read `done` themselves.
//
// cg_solve_fsai is the same loop again with z = GT (G r) (include/spmv/fsai.h): two launches of the
// direct vector-CSR kernel (launch_csr_vector, kernels.hip) through a fifth workspace vector t; they do not read `done`.
//
// The host side is built from solver_common.h's parts (Workspace and its mirror, TriangularPair, TiledEngine,
// diag_kernel); what is here is this solver's checks, its workspace layout, its launches and its result.  The state and
// the kernels that do not read the matrix (cg_start_kernel, cg_update_kernel, cg_rz_kernel, cg_direction_kernel) are
// cg_impl.h's, shared with cg_bsr.hip.
#include "amg_impl.h"
#include "cg_impl.h"
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"
#include "tiled.h"
#include "spmv/cg.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

// r0 = b - A x0, p0 = z0 = r0 * dinv, and the block partials of r.z, r.r and b.b -> part[3 * block].
template <int LANES>
__global__ __launch_bounds__(kBlock)
void cg_init_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                    const float* __restrict__ vals, const float* __restrict__ b, const float* __restrict__ x,
                    const float* __restrict__ dinv, float* __restrict__ r, float* __restrict__ p,
                    double* __restrict__ part) {
    double rz = 0.0, rr = 0.0, bb = 0.0, unused = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        const float bi = b[row];
        const float ri = __fsub_rn(bi, acc);
        const float zi = dinv ? __fmul_rn(ri, dinv[row]) : ri;
        r[row] = ri;
        p[row] = zi;
        rz += prod64(ri, zi);
        rr += prod64(ri, ri);
        bb += prod64(bi, bi);
    });
    block_sum2(rz, rr);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = rz;
        part[3 * blockIdx.x + 1] = rr;
    }
    block_sum2(bb, unused);
    if (threadIdx.x == 0) part[3 * blockIdx.x + 2] = bb;
}

// q = A p and the block partials of p.q -> part[block].  p_i is the row's own entry: q is not read back.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void cg_spmv_dot(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                 const float* __restrict__ vals, const float* __restrict__ p, float* __restrict__ q,
                 const CgState* __restrict__ state, double* __restrict__ part) {
    if (state->done) return;
    double pq = 0.0, unused = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, p, [&](long long row, float acc) {
        q[row] = acc;
        pq += prod64(p[row], acc);
    });
    block_sum2(pq, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = pq;
}

// Block partials of p.q -> part[block] (tiled engine: q came from tiled_spmv).
__global__ __launch_bounds__(kBlock)
void cg_dot_kernel(int n, const float* __restrict__ p, const float* __restrict__ q,
                   const CgState* __restrict__ state, double* __restrict__ part) {
    if (state->done) return;
    double pq = 0.0, unused = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        pq += prod64(p[i], q[i]);
    }
    block_sum2(pq, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = pq;
}

hipError_t init(int lanes, const CSRMatrix* A, const float* b, const float* x, const float* dinv, float* r,
                float* p, double* part, int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        cg_init_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                  A->d_col_indices, A->d_values, b, x, dinv, r, p,
                                                                  part);
        return hipGetLastError();
    });
}

hipError_t spmv_dot(int lanes, const CSRMatrix* A, const float* p, float* q, const CgState* state, double* part,
                    int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        cg_spmv_dot<decltype(L)::value><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                               A->d_col_indices, A->d_values, p, q, state, part);
        return hipGetLastError();
    });
}

// What gives z: the diagonal inside the step kernels (cg_solve: cfg.preconditioner picks NONE or JACOBI), or a stored z
// from M = L L^T of the factor matrix F (cg_solve_ic) or from one V-cycle of the hierarchy H (cg_solve_amg); the last
// two do not read cfg.preconditioner.  FSAI (cg_solve_fsai): a stored z = FT (F t), t = F r, two direct vector-CSR
// SpMVs with F = G and FT = GT; it does not read cfg.preconditioner either.
enum class Precond { DIAGONAL, IC, AMG, FSAI };

CGResult solve(const CSRMatrix* A, Precond precond, const CSRMatrix* F, const CSRMatrix* FT, const AMGHierarchy* H,
               const float* d_b, float* d_x, const CGConfig* config) {
    const bool with_ic = precond == Precond::IC;
    const bool with_amg = precond == Precond::AMG;
    const bool with_fsai = precond == Precond::FSAI;
    const bool stored_z = with_ic || with_amg || with_fsai;
    CGResult result;
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
    const CGConfig defaults;
    const CGConfig& cfg = config ? *config : defaults;
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 ||
        (!stored_z && cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI) ||
        cfg.engine < -1 || cfg.engine > 1) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const int n = A->num_rows;
    if (ranges_overlap(d_b, d_x, n)) return fail(SpMVError::INVALID_ARGUMENT);
    if (with_ic) {
        if (!F) return fail(SpMVError::INVALID_ARGUMENT);
        if (F->num_rows != F->num_cols || F->num_rows != n) return fail(SpMVError::INVALID_DIMENSION);
        if (!device_arrays(F)) return fail(SpMVError::INVALID_FORMAT);
    }
    if (with_amg) {
        if (!H || H->levels.empty()) return fail(SpMVError::INVALID_ARGUMENT);
        if (H->num_rows != n) return fail(SpMVError::INVALID_DIMENSION);
        if (H->config.pre_sweeps != H->config.post_sweeps) return fail(SpMVError::INVALID_ARGUMENT);
    }
    if (with_fsai) {
        if (!F || !FT) return fail(SpMVError::INVALID_ARGUMENT);
        for (const CSRMatrix* M : {F, FT}) {
            if (M->num_rows != M->num_cols || M->num_rows != n) return fail(SpMVError::INVALID_DIMENSION);
        }
        if (!device_arrays(F) || !device_arrays(FT)) return fail(SpMVError::INVALID_FORMAT);
    }

    const TraceRange range(with_ic ? "spmv:cg_solve_ic" : with_amg ? "spmv:cg_solve_amg" :
                           with_fsai ? "spmv:cg_solve_fsai" : "spmv:cg_solve");
    hipStream_t stream = current_stream();
    const bool jacobi = !stored_z && cfg.preconditioner == CGConfig::JACOBI;

    TriangularPair ic;              // M = L L^T: the lower solve reads L's stored diagonal
    if (with_ic) {
        const int status = ic.build(F, 0, stream);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }
    const int amg_lanes = with_amg ? amg_forced_lanes() : 0;
    TiledEngine engine(A, cfg.engine, stream);

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const size_t pq_count = static_cast<size_t>(std::max(row_grid, vgrid));
    const size_t rr_count = 2 * static_cast<size_t>(vgrid);
    const size_t init_count = 3 * static_cast<size_t>(row_grid);

    Workspace<CgState> ws;          // r, p, q, and dinv (JACOBI) or z (IC, AMG, FSAI); FSAI: t = G r as well
    const size_t len = static_cast<size_t>(n);
    if (!ws.allocate((with_fsai ? 5 : 4) * len, pq_count + rr_count + init_count)) return fail(SpMVError::CUDA_MALLOC);
    float* r = ws.vec;
    float* p = ws.vec + len;
    float* q = ws.vec + 2 * len;
    float* dinv = jacobi ? ws.vec + 3 * len : nullptr;
    float* z = stored_z ? ws.vec + 3 * len : nullptr;
    float* t = with_fsai ? ws.vec + 4 * len : nullptr;
    // FSAI: the lanes of each factor's own mean row length; the launches are the direct vector kernel's, not a dispatch
    const int g_lanes = with_fsai ? pick_lanes_per_row(static_cast<float>(F->nnz) / n) : 0;
    const int gt_lanes = with_fsai ? pick_lanes_per_row(static_cast<float>(FT->nnz) / n) : 0;
    double* pq_part = ws.part;
    double* rr_part = ws.part + pq_count;
    double* init_part = rr_part + rr_count;
    // out = M^-1 in.  IC: both triangular solves.  AMG: one V-cycle, whose kernels read `done`.  FSAI: two SpMVs,
    // which like the triangular solves do not read `done`: after it r no longer changes and they rewrite the same z.
    const auto apply_stored = [&](const float* in, float* out) -> bool {
        if (with_amg) return amg_vcycle(*H, in, out, &ws.state->done, amg_lanes, stream) == hipSuccess;
        if (with_fsai) {
            return launch_csr_vector(F, in, t, g_lanes, stream) == hipSuccess &&
                   launch_csr_vector(FT, t, out, gt_lanes, stream) == hipSuccess;
        }
        return ic.apply(in, out, stream);
    };

    // setup: diagonal (JACOBI; of F, only its check), r0 / p0 and their dots, the state; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(CgState), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (with_ic) ok = ok && launch_diag<DiagRule::POSITIVE_FINITE>(F, nullptr, bad, stream) == hipSuccess;
    if (jacobi) ok = ok && launch_diag<DiagRule::POSITIVE>(A, dinv, bad, stream) == hipSuccess;
    ok = ok && init(lanes, A, d_b, d_x, dinv, r, p, init_part, row_grid, stream) == hipSuccess;
    if (ok && stored_z) {
        // the init kernel left p0 = r0 and r0.r0 in the r.z slot: z0 = M^-1 r0, the true r0.z0 over it, p0 = z0
        ok = apply_stored(r, z);
        if (ok) {
            cg_rz_kernel<<<row_grid, kBlock, 0, stream>>>(n, r, z, ws.state, init_part, 3);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(p, z, len * sizeof(float), hipMemcpyDeviceToDevice, stream) == hipSuccess;
        }
    }
    if (ok) {
        cg_start_kernel<<<1, kBlock, 0, stream>>>(init_part, row_grid, cfg.tolerance, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (ws.pinned[0].bad_diagonal) return fail(SpMVError::INVALID_ARGUMENT);
    if (ws.pinned[0].zero_b) {
        if (!zero_solution(d_x, len, stream)) return fail(SpMVError::KERNEL_LAUNCH);
        result.converged = 1;
        return result;
    }

    if (!ws.pinned[0].done) {
        EventPair& ev = thread_events();
        ok = hipEventRecord(ev.start, stream) == hipSuccess;
        for (int iter = 0; ok && iter < cfg.max_iterations; ++iter) {
            if (!engine.build_if_due(iter, ws, stream, ok)) break;
            const TraceRange step_range("spmv:cg_step");
            int pq_parts = row_grid;
            const TiledEngine::Spmv spmv = engine.spmv(p, q, stream);
            ok = ok && spmv != TiledEngine::Spmv::FAILED;
            if (spmv == TiledEngine::Spmv::TILED) {
                cg_dot_kernel<<<vgrid, kBlock, 0, stream>>>(n, p, q, ws.state, pq_part);
                ok = hipGetLastError() == hipSuccess;
                pq_parts = vgrid;
            } else if (ok) {
                ok = spmv_dot(lanes, A, p, q, ws.state, pq_part, row_grid, stream) == hipSuccess;
            }
            if (ok && stored_z) {
                cg_update_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, p, q, nullptr, d_x, r, ws.state, pq_part,
                                                                     pq_parts, rr_part);
                ok = hipGetLastError() == hipSuccess && apply_stored(r, z);
            }
            if (ok) {
                if (stored_z) {
                    cg_rz_kernel<<<vgrid, kBlock, 0, stream>>>(n, r, z, ws.state, rr_part, 2);
                    cg_direction_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, z, nullptr, p, ws.state, rr_part,
                                                                            vgrid);
                } else {
                    cg_update_kernel<false><<<vgrid, kBlock, 0, stream>>>(n, iter, p, q, dinv, d_x, r, ws.state,
                                                                          pq_part, pq_parts, rr_part);
                    cg_direction_kernel<false><<<vgrid, kBlock, 0, stream>>>(n, iter, r, dinv, p, ws.state, rr_part,
                                                                             vgrid);
                }
                ok = hipGetLastError() == hipSuccess && ws.publish(iter, sizeof(CgState), stream);
            }
            if (ok && iter >= 1) {
                const CgState* seen = ws.wait_previous(iter);
                ok = seen != nullptr;
                if (ok && seen->done) break;
            }
        }
        if (!ws.finish_timed(ok, ev, stream, &result.elapsed_ms)) return fail(SpMVError::KERNEL_LAUNCH);
    }
    const CgState& final_state = ws.pinned[0];
    result.iterations = final_state.iterations;
    result.relative_residual = final_state.relative_residual;
    result.converged = final_state.converged;
    result.breakdown = final_state.breakdown;
    return result;
}

} // namespace
} // namespace detail

CGResult cg_solve(const CSRMatrix* A, const float* d_b, float* d_x, const CGConfig* config) {
    return detail::solve(A, detail::Precond::DIAGONAL, nullptr, nullptr, nullptr, d_b, d_x, config);
}

CGResult cg_solve_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_b, float* d_x, const CGConfig* config) {
    return detail::solve(A, detail::Precond::IC, F, nullptr, nullptr, d_b, d_x, config);
}

CGResult cg_solve_amg(const CSRMatrix* A, const AMGHierarchy* H, const float* d_b, float* d_x, const CGConfig* config) {
    return detail::solve(A, detail::Precond::AMG, nullptr, nullptr, H, d_b, d_x, config);
}

CGResult cg_solve_fsai(const CSRMatrix* A, const CSRMatrix* G, const CSRMatrix* GT, const float* d_b, float* d_x,
                       const CGConfig* config) {
    return detail::solve(A, detail::Precond::FSAI, G, GT, nullptr, d_b, d_x, config);
}

} // namespace spmv
