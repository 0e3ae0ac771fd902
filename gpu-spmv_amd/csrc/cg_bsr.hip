// cg_bsr.hip — conjugate gradients on a BSRMatrix with a block-Jacobi preconditioner (include/spmv/cg.h cg_solve_bsr,
// include/spmv/bsr.h bsr_diag_inverse_gpu / bsr_diag_apply) or with a block IC(0) factor
// (cg_solve_bsr_ic: cg.hip's stored-z step on this file's product, the solves of bsr_tri.hip).
//
// The loop is cg.hip's: the scalars live in a device CgState, every loop kernel returns at once when `done` is set, and
// the host reads the two-deep pinned mirror of the state.  z = M^-1 r is a stored vector for every preconditioner, so
// the state, its start, the r.z partials of setup and the direction step are cg_impl.h's, shared with cg.hip.  Per step
// three launches, whatever the block size and the preconditioner:
//   cg_bsr_spmv_dot<B, LANES, WIDE>  q = A p by the lane-group walk of bsr_device.h and the block partials of p.q
//   cg_bsr_update<B>                 every workgroup folds the p.q partials, then x += alpha p, r -= alpha q, z = M^-1 r
//                                    and the block partials of r.z and r.r.  One thread per scalar row, T = kBlock -
//                                    kBlock % B rows a trip so that no block straddles two workgroups; the new r of a
//                                    block goes through LDS, because r is updated in place and a thread must not read a
//                                    neighbour's r from memory in the launch that writes it
//   cg_direction_kernel<true>        beta, the stop test, p = z + beta p
// M^-1 is nothing (NONE: z = r), a per-row 1 / d (JACOBI, d the (k,k) entry of the stored diagonal block) or the b x b
// inverses of the diagonal blocks (BLOCK_JACOBI), applied by bsr_diag_impl.h's ordered sum, multiply and add rounded
// separately.  The inverses come from one launch, one lane per block row, every fp64 operation rounded on its own: the
// bits of bsr_diag_inverse_cpu on every run.
// Dot products accumulate fp64 products of the fp32 entries; no float atomics anywhere.
#include "bsr_device.h"
#include "bsr_diag_impl.h"
#include "bsr_impl.h"
#include "bsr_tri_impl.h"
#include "cg_impl.h"
#include "device_common.h"
#include "internal.h"
#include "solver_common.h"
#include "spmv/bsr.h"
#include "spmv/cg.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace spmv {
namespace detail {
namespace bsr {

namespace {

using namespace dev;
using namespace solver;

// rows a workgroup of cg_bsr_update and of the setup kernels takes per trip: whole blocks only
template <int B>
constexpr int kTripRows = kBlock - kBlock % B;

// ---- the diagonal blocks ---------------------------------------------------------------------------------------
// inv[I] = fl32(D_I^-1), one lane per block row; *flag = 1 for a block row without a stored diagonal block or with a
// pivot that is not > 0 or not finite (every writer stores the same 1)
template <int B>
__global__ __launch_bounds__(kBlock)
void bsr_diag_inverse_kernel(const int* __restrict__ brp, const int* __restrict__ bc, const float* __restrict__ bv,
                             int n, int block_rows, float* __restrict__ inv, int* __restrict__ flag) {
    bool bad = false;
    for (long long I = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; I < block_rows;
         I += static_cast<long long>(gridDim.x) * kBlock) {
        const int at = find_block(bc, brp[I], brp[I + 1], static_cast<int>(I));
        if (at < 0) {
            bad = true;
            continue;
        }
        const int size = static_cast<int>(min(static_cast<long long>(B), n - I * B));
        if (!diag_block_inverse<B>(bv + static_cast<long long>(at) * (B * B), size, inv + I * (B * B))) bad = true;
    }
    if (bad) *flag = 1;
}

// JACOBI on a BSR matrix: dinv[i] = 1 / the (k,k) entry of the stored diagonal block of row i = I * B + k, 0 and
// *flag = 1 where the block is missing or the entry is not > 0 (cg_solve's rule).  One thread per scalar row.
template <int B>
__global__ __launch_bounds__(kBlock)
void bsr_diag_scalar_kernel(const int* __restrict__ brp, const int* __restrict__ bc, const float* __restrict__ bv,
                            int n, float* __restrict__ dinv, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int I = static_cast<int>(i / B), k = static_cast<int>(i % B);
        const int at = find_block(bc, brp[I], brp[I + 1], I);
        const float d = at >= 0 ? bv[(static_cast<long long>(at) * B + k) * B + k] : 0.0f;
        const bool ok = at >= 0 && d > 0.0f;
        dinv[i] = ok ? __fdiv_rn(1.0f, d) : 0.0f;
        bad = bad || !ok;
    }
    if (bad) *flag = 1;
}

// row i of the inverses, B floats at inv + i * B.  ALIGNED: inv is 16-byte aligned (the solver's own array).
template <int B, bool ALIGNED>
__device__ __forceinline__ void load_inv_row(const float* __restrict__ inv, long long i, float (&row)[B]) {
    const float* at = inv + i * B;
    if constexpr (ALIGNED && B % 4 == 0) {
#pragma unroll
        for (int k = 0; k < B / 4; ++k) {
            const f32x4 t = reinterpret_cast<const f32x4*>(at)[k];
            row[4 * k] = t[0];
            row[4 * k + 1] = t[1];
            row[4 * k + 2] = t[2];
            row[4 * k + 3] = t[3];
        }
    } else if constexpr (ALIGNED && B == 2) {
        const float2 t = *reinterpret_cast<const float2*>(at);
        row[0] = t.x;
        row[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < B; ++k) row[k] = at[k];
    }
}

// z = M^-1 r out of place (setup, and bsr_diag_apply): inv the block inverses, else dinv a per-row factor, else z = r.
// r is not written in this launch, so a thread reads its block's r from memory.
template <int B, bool ALIGNED>
__global__ __launch_bounds__(kBlock)
void bsr_diag_apply_kernel(int n, const float* __restrict__ inv, const float* __restrict__ dinv,
                           const float* __restrict__ r, float* __restrict__ z) {
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float zi;
        if (inv) {
            const long long first = i - i % B;
            float row[B], rb[B];
            load_inv_row<B, ALIGNED>(inv, i, row);
#pragma unroll
            for (int c = 0; c < B; ++c) rb[c] = first + c < n ? r[first + c] : 0.0f;
            zi = diag_apply_row<B>(row, rb, first, n);
        } else {
            zi = dinv ? __fmul_rn(r[i], dinv[i]) : r[i];
        }
        z[i] = zi;
    }
}

// ---- the solver's kernels --------------------------------------------------------------------------------------
// r0 = b - A x0 and the block partials of r.r and b.b -> part[3 * block + 1], part[3 * block + 2] (r.z follows from
// cg_rz_kernel once z0 is there)
template <int B, int LANES, bool WIDE>
__global__ __launch_bounds__(kBlock)
void cg_bsr_init(const int* __restrict__ brp, const int* __restrict__ bc, const float* __restrict__ bv, int n,
                 int block_rows, const float* __restrict__ b, const float* __restrict__ x, float* __restrict__ r,
                 double* __restrict__ part) {
    double rr = 0.0, bb = 0.0;
    for_each_block_row_dot<B, LANES, WIDE>(brp, bc, bv, x, n, n, block_rows, [&](long long row, float sum) {
        const float bi = b[row];
        const float ri = __fsub_rn(bi, sum);
        r[row] = ri;
        rr += prod64(ri, ri);
        bb += prod64(bi, bi);
    });
    block_sum2(rr, bb);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x + 1] = rr;
        part[3 * blockIdx.x + 2] = bb;
    }
}

// q = A p and the block partials of p.q -> part[block]: the lanes that store q[row] hold p[row] * q[row] as well
template <int B, int LANES, bool WIDE>
__global__ __launch_bounds__(kBlock)
void cg_bsr_spmv_dot(const int* __restrict__ brp, const int* __restrict__ bc, const float* __restrict__ bv, int n,
                     int block_rows, const float* __restrict__ p, float* __restrict__ q,
                     const CgState* __restrict__ state, double* __restrict__ part) {
    if (state->done) return;
    double pq = 0.0, unused = 0.0;
    for_each_block_row_dot<B, LANES, WIDE>(brp, bc, bv, p, n, n, block_rows, [&](long long row, float sum) {
        q[row] = sum;
        pq += prod64(p[row], sum);
    });
    block_sum2(pq, unused);
    if (threadIdx.x == 0) part[blockIdx.x] = pq;
}

// alpha = rz / p.q; x += alpha p; r -= alpha q; z = M^-1 r; partials of r.z and r.r -> part_out[2 * block].
// A trip of a workgroup covers kTripRows<B> consecutive rows, whole blocks: the new r goes to memory and into LDS,
// and after the barrier each thread forms z_i from its block's B values there.  The LDS line alternates with the trip,
// so one barrier a trip is enough: a thread that writes line t & 1 for trip t + 2 has passed trip t + 1's barrier, which
// every thread reaches only after its reads of trip t.
template <int B>
__global__ __launch_bounds__(kBlock)
void cg_bsr_update(int n, int step, const float* __restrict__ p, const float* __restrict__ q,
                   const float* __restrict__ inv, const float* __restrict__ dinv, float* __restrict__ x,
                   float* __restrict__ r, float* __restrict__ z, CgState* __restrict__ state,
                   const double* __restrict__ pq_part, int pq_count, double* __restrict__ part_out) {
    constexpr int T = kTripRows<B>;
    __shared__ float s_r[2][kBlock];
    if (state->done) return;
    double pq = 0.0, unused = 0.0;
    fold_partials(pq_part, pq_count, 1, pq, unused);
    if (!(pq > 0.0)) {             // A is not SPD (or p.q is not finite): x stays at the last good iterate
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state->breakdown = 1;
            state->done = 1;
        }
        return;
    }
    const float alpha = static_cast<float>(state->rz[step & 1] / pq);
    const int first_in_block = threadIdx.x - threadIdx.x % B;
    double rz = 0.0, rr = 0.0;
    int trip = 0;
    for (long long base = static_cast<long long>(blockIdx.x) * T; base < n;
         base += static_cast<long long>(gridDim.x) * T, ++trip) {
        float* line = s_r[trip & 1];
        const long long i = base + threadIdx.x;
        const bool active = threadIdx.x < T && i < n;
        float ri = 0.0f;
        if (active) {
            x[i] = __builtin_fmaf(alpha, p[i], x[i]);
            ri = __builtin_fmaf(-alpha, q[i], r[i]);
            r[i] = ri;
        }
        line[threadIdx.x] = ri;
        __syncthreads();
        if (active) {
            float zi;
            if (inv) {
                float row[B], rb[B];
                load_inv_row<B, true>(inv, i, row);
#pragma unroll
                for (int c = 0; c < B; ++c) rb[c] = line[first_in_block + c];
                zi = diag_apply_row<B>(row, rb, base + first_in_block, n);
            } else {
                zi = dinv ? __fmul_rn(ri, dinv[i]) : ri;
            }
            z[i] = zi;
            rz += prod64(ri, zi);
            rr += prod64(ri, ri);
        }
    }
    block_sum2(rz, rr);
    if (threadIdx.x == 0) {
        part_out[2 * blockIdx.x] = rz;
        part_out[2 * blockIdx.x + 1] = rr;
    }
}

// ---- launches ----
hipError_t launch_inverse(const BSRMatrix* A, float* inv, int* flag, hipStream_t s) {
    return with_block_dim(A->block_dim, [&](auto Bc) {
        bsr_diag_inverse_kernel<decltype(Bc)::value><<<vec_grid(A->num_block_rows), kBlock, 0, s>>>(
            A->d_block_row_ptrs, A->d_block_cols, A->d_values, A->num_rows, A->num_block_rows, inv, flag);
        return hipGetLastError();
    });
}

hipError_t launch_scalar_diag(const BSRMatrix* A, float* dinv, int* flag, hipStream_t s) {
    return with_block_dim(A->block_dim, [&](auto Bc) {
        bsr_diag_scalar_kernel<decltype(Bc)::value><<<vec_grid(A->num_rows), kBlock, 0, s>>>(
            A->d_block_row_ptrs, A->d_block_cols, A->d_values, A->num_rows, dinv, flag);
        return hipGetLastError();
    });
}

template <bool ALIGNED>
hipError_t launch_apply(int block_dim, int n, const float* inv, const float* dinv, const float* r, float* z,
                        hipStream_t s) {
    return with_block_dim(block_dim, [&](auto Bc) {
        bsr_diag_apply_kernel<decltype(Bc)::value, ALIGNED><<<vec_grid(n), kBlock, 0, s>>>(n, inv, dinv, r, z);
        return hipGetLastError();
    });
}

// launch(B, LANES, WIDE as integral constants) for A's block size, the lane count and the alignment of A's values
template <class Launch>
hipError_t with_walk(const BSRMatrix* A, int lanes, Launch&& launch) {
    const bool wide = aligned16(A->d_values);
    return with_block_dim(A->block_dim, [&](auto Bc) {
        constexpr int B = decltype(Bc)::value;
        return with_lanes(lanes, [&](auto L) {
            if (B * B % 4 == 0 && wide) return launch(Bc, L, std::integral_constant<bool, B * B % 4 == 0>{});
            return launch(Bc, L, std::false_type{});
        });
    });
}

hipError_t launch_update(const BSRMatrix* A, int grid, int step, const float* p, const float* q, const float* inv,
                         const float* dinv, float* x, float* r, float* z, CgState* state, const double* pq_part,
                         int pq_count, double* part_out, hipStream_t s) {
    return with_block_dim(A->block_dim, [&](auto Bc) {
        cg_bsr_update<decltype(Bc)::value><<<grid, kBlock, 0, s>>>(A->num_rows, step, p, q, inv, dinv, x, r, z, state,
                                                                   pq_part, pq_count, part_out);
        return hipGetLastError();
    });
}

// F == nullptr: cg_solve_bsr, M^-1 from cfg.preconditioner.  with_ic: cg_solve_bsr_ic, z = L^-T (L^-1 r) by the two block
// triangular solves with the factor matrix F (bsr_tri.hip), a stored z between cg.hip's update and r.z kernels.
CGResult solve(const BSRMatrix* A, bool with_ic, const BSRMatrix* F, const float* d_b, float* d_x,
               const CGConfig* config) {
    CGResult result;
    const auto fail = [&result](SpMVError e) {
        result.error_code = code(e);
        return result;
    };
    const CGConfig defaults;
    CGConfig cfg = config ? *config : defaults;
    if (with_ic) cfg.preconditioner = CGConfig::NONE;      // not read: the factor is the preconditioner
    bool nothing = false;
    int status = cg_check(A, d_b, d_x, cfg, &nothing);
    if (status != 0) return fail(static_cast<SpMVError>(status));
    if (nothing) {
        result.converged = 1;
        return result;
    }
    if (with_ic) {
        status = cg_ic_check(A, F);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }

    const TraceRange range(with_ic ? "spmv:cg_solve_bsr_ic" : "spmv:cg_solve_bsr");
    hipStream_t stream = current_stream();
    // M = L L^T: both schedules of F's block pattern, which validate it before any kernel walks it
    ScheduleRef lower, upper;
    int lower_lanes = 1, upper_lanes = 1;
    if (with_ic) {
        float analysis_ms = 0.0f;
        status = tri_schedule_for(F, SpTRSVConfig::LOWER, stream, &lower, &analysis_ms);
        if (status == 0) status = tri_schedule_for(F, SpTRSVConfig::UPPER, stream, &upper, &analysis_ms);
        if (status != 0) return fail(static_cast<SpMVError>(status));
        if (lower->first_missing_diagonal >= 0 || lower->first_unsorted_row >= 0) {
            return fail(SpMVError::INVALID_ARGUMENT);
        }
        lower_lanes = tri_lanes(*lower, false);
        upper_lanes = tri_lanes(*upper, false);
    }
    // z = L^-T (L^-1 in): LOWER into out, then UPPER in place.  Like cg.hip's triangular solves they do not read `done`:
    // after it r no longer changes and they rewrite the same z.
    const auto apply_factor = [&](const float* in, float* out) {
        return launch_sptrsv_bsr(*lower, F, in, out, SpTRSVConfig::LOWER, 0, false, lower_lanes, stream) == hipSuccess &&
               launch_sptrsv_bsr(*upper, F, out, out, SpTRSVConfig::UPPER, 0, false, upper_lanes, stream) == hipSuccess;
    };
    const int n = A->num_rows, b = A->block_dim, block_rows = A->num_block_rows;
    const bool jacobi = cfg.preconditioner == CGConfig::JACOBI;
    const bool block_jacobi = cfg.preconditioner == CGConfig::BLOCK_JACOBI;

    const int lanes = product_lanes(A);
    const int row_grid = capped_grid(block_rows, kBlock / lanes);
    const int update_grid = capped_grid(n, kBlock - kBlock % b, kVecBlocks);
    const int vgrid = vec_grid(n);
    const size_t pq_count = static_cast<size_t>(row_grid);
    const size_t rr_count = 2 * static_cast<size_t>(std::max(update_grid, vgrid));
    const size_t init_count = 3 * static_cast<size_t>(row_grid);

    Workspace<CgState> ws;          // r, p, q, z, and dinv (JACOBI) or the block inverses (BLOCK_JACOBI)
    const size_t len = static_cast<size_t>(n);
    const size_t extra = jacobi ? len : block_jacobi ? static_cast<size_t>(block_rows) * b * b : 0;
    if (!ws.allocate(4 * len + extra, pq_count + rr_count + init_count)) return fail(SpMVError::CUDA_MALLOC);
    float* r = ws.vec;
    float* p = ws.vec + len;
    float* q = ws.vec + 2 * len;
    float* z = ws.vec + 3 * len;
    float* dinv = jacobi ? ws.vec + 4 * len : nullptr;
    float* inv = block_jacobi ? ws.vec + 4 * len : nullptr;      // 16 * len bytes in: 16-byte aligned
    double* pq_part = ws.part;
    double* rr_part = ws.part + pq_count;
    double* init_part = rr_part + rr_count;

    // setup: the inverses or the diagonal, r0 and its dots, z0 = M^-1 r0, r0.z0, p0 = z0, the state; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(CgState), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (block_jacobi) ok = ok && launch_inverse(A, inv, bad, stream) == hipSuccess;
    if (jacobi) ok = ok && launch_scalar_diag(A, dinv, bad, stream) == hipSuccess;
    if (with_ic) ok = ok && launch_factor_diag_check(F, bad, stream) == hipSuccess;
    ok = ok && with_walk(A, lanes, [&](auto Bc, auto L, auto W) {
        cg_bsr_init<decltype(Bc)::value, decltype(L)::value, decltype(W)::value><<<row_grid, kBlock, 0, stream>>>(
            A->d_block_row_ptrs, A->d_block_cols, A->d_values, n, block_rows, d_b, d_x, r, init_part);
        return hipGetLastError();
    }) == hipSuccess;
    ok = ok && (with_ic ? apply_factor(r, z) : launch_apply<true>(b, n, inv, dinv, r, z, stream) == hipSuccess);
    if (ok) {
        cg_rz_kernel<<<row_grid, kBlock, 0, stream>>>(n, r, z, ws.state, init_part, 3);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(p, z, len * sizeof(float), hipMemcpyDeviceToDevice, stream) == hipSuccess;
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
            const TraceRange step_range("spmv:cg_bsr_step");
            ok = with_walk(A, lanes, [&](auto Bc, auto L, auto W) {
                cg_bsr_spmv_dot<decltype(Bc)::value, decltype(L)::value, decltype(W)::value>
                    <<<row_grid, kBlock, 0, stream>>>(A->d_block_row_ptrs, A->d_block_cols, A->d_values, n, block_rows, p,
                                                      q, ws.state, pq_part);
                return hipGetLastError();
            }) == hipSuccess;
            if (ok && with_ic) {
                cg_update_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, p, q, nullptr, d_x, r, ws.state, pq_part,
                                                                     row_grid, rr_part);
                ok = hipGetLastError() == hipSuccess && apply_factor(r, z);
                if (ok) cg_rz_kernel<<<vgrid, kBlock, 0, stream>>>(n, r, z, ws.state, rr_part, 2);
            } else {
                ok = ok && launch_update(A, update_grid, iter, p, q, inv, dinv, d_x, r, z, ws.state, pq_part, row_grid,
                                         rr_part, stream) == hipSuccess;
            }
            if (ok) {
                cg_direction_kernel<true><<<vgrid, kBlock, 0, stream>>>(n, iter, z, nullptr, p, ws.state, rr_part,
                                                                        with_ic ? vgrid : update_grid);
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

} // namespace bsr
} // namespace detail

int bsr_diag_inverse_gpu(const BSRMatrix* A, float* d_inv) {
    using namespace detail;
    const int status = bsr::diag_check(A, d_inv, true);
    if (status != 0) return status;
    if (A->num_rows == 0) return 0;
    const TraceRange range("spmv:bsr_diag_inverse_gpu");
    hipStream_t s = current_stream();
    DevBuf<int> flag;
    if (dev_alloc(&flag, 1) != hipSuccess) return fail(SpMVError::CUDA_MALLOC);
    int bad = 0;
    bool ok = hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
              bsr::launch_inverse(A, d_inv, flag.get(), s) == hipSuccess &&
              hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok) return fail(SpMVError::KERNEL_LAUNCH);
    return bad ? code(SpMVError::INVALID_ARGUMENT) : 0;
}

int bsr_diag_apply(const BSRMatrix* A, const float* d_inv, const float* d_r, float* d_z) {
    using namespace detail;
    if (!A || !d_inv || !d_r || !d_z) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (!bsr::shape_ok(A)) return code(SpMVError::INVALID_FORMAT);
    if (A->num_rows == 0) return 0;
    const TraceRange range("spmv:bsr_diag_apply");
    hipStream_t s = current_stream();
    if (bsr::launch_apply<false>(A->block_dim, A->num_rows, d_inv, nullptr, d_r, d_z, s) != hipSuccess) {
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    return stream_finished(s);
}

CGResult cg_solve_bsr(const BSRMatrix* A, const float* d_b, float* d_x, const CGConfig* config) {
    return detail::bsr::solve(A, false, nullptr, d_b, d_x, config);
}

CGResult cg_solve_bsr_ic(const BSRMatrix* A, const BSRMatrix* F, const float* d_b, float* d_x, const CGConfig* config) {
    return detail::bsr::solve(A, true, F, d_b, d_x, config);
}

} // namespace spmv
