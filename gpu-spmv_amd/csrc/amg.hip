// amg.hip — the V-cycle of the aggregation AMG (include/spmv/amg.h): damped Jacobi sweeps, the fused
// residual + restriction, the prolongation + correction and the dense coarse solve, all in stream order on one stream.
//
// Launches of one cycle, per level below the coarsest: pre_sweeps (amg_scale_kernel, then amg_sweep_kernel each),
// one amg_restrict_kernel, one amg_correct_kernel, post_sweeps amg_sweep_kernel; on the coarsest level one
// amg_dense_kernel, or coarse_sweeps smoother launches.  Every kernel reads `done` first (null inside amg_apply; the
// `done` of the CG state inside cg_solve_amg) and returns at once when it is set.  The rows of a level are spread over
// groups of LANES lanes as in cg_spmv_dot; the restriction gives one group to an aggregate, which walks its member
// rows one after another and adds their residuals in fp32 in member order, so the fine residual is never stored.
//
// A smoothed hierarchy has real matrices for both transfers: its levels take, in place of the two
// launches above, one amg_residual_kernel (r = f - A x, stored), one amg_restrict_weighted_kernel (PT r) and one
// amg_prolong_kernel (x += P e), each the same row sweep over its own matrix at its own lane count.
#include "amg_impl.h"
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"

#include <hip/hip_runtime.h>

#include <vector>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

__device__ __forceinline__ bool finished(const int* __restrict__ done) { return done && *done; }

// x_i = wd_i * f_i: one damped Jacobi sweep from a zero guess
__global__ __launch_bounds__(kBlock)
void amg_scale_kernel(int n, const float* __restrict__ wd, const float* __restrict__ f, float* __restrict__ x,
                      const int* __restrict__ done) {
    if (finished(done)) return;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        x[i] = __fmul_rn(wd[i], f[i]);
    }
}

// x'_i = fmaf(wd_i, f_i - (A x)_i, x_i); x_out is another array than x_in
template <int LANES>
__global__ __launch_bounds__(kBlock)
void amg_sweep_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                      const float* __restrict__ vals, const float* __restrict__ wd, const float* __restrict__ f,
                      const float* __restrict__ x_in, float* __restrict__ x_out, const int* __restrict__ done) {
    if (finished(done)) return;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x_in, [&](long long row, float acc) {
        x_out[row] = __builtin_fmaf(wd[row], __fsub_rn(f[row], acc), x_in[row]);
    });
}

// f_coarse[a] = sum over the members i of aggregate a (member_ptr / members: the structure of P^T, rows ascending) of
// f_i - (A x)_i.  One lane group per aggregate; the trip count is made uniform over the wavefront so that the
// cross-lane sum is reached by all of its lanes together.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void amg_restrict_kernel(int num_aggregates, long long nnz, const int* __restrict__ row_ptrs,
                         const int* __restrict__ cols, const float* __restrict__ vals,
                         const int* __restrict__ member_ptr, const int* __restrict__ members,
                         const float* __restrict__ f, const float* __restrict__ x, float* __restrict__ f_coarse,
                         const int* __restrict__ done) {
    if (finished(done)) return;
    constexpr int kGroupsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (long long first = static_cast<long long>(blockIdx.x) * kGroupsPerBlock; first < num_aggregates;
         first += static_cast<long long>(gridDim.x) * kGroupsPerBlock) {
        const long long a = first + slot;
        int begin = 0, count = 0;
        if (a < num_aggregates) {
            begin = member_ptr[a];
            count = member_ptr[a + 1] - begin;
        }
        float sum = 0.0f;
        for (int m = 0; __any(m < count); ++m) {
            const bool live = m < count;
            int row = 0;
            float acc = 0.0f;
            if (live) {
                row = members[begin + m];
                acc = row_partial_dot<LANES>(row_ptrs[row], row_ptrs[row + 1], lane, nnz, cols, vals, x);
            }
            acc = group_sum<LANES>(acc);
            if (live) sum = __fadd_rn(sum, __fsub_rn(f[row], acc));
        }
        if (lane == 0 && a < num_aggregates) f_coarse[a] = sum;
    }
}

// x_out_i = x_in_i + e[aggregate_i]; x_out may be x_in itself
__global__ __launch_bounds__(kBlock)
void amg_correct_kernel(int n, const int* __restrict__ aggregate, const float* __restrict__ e, const float* x_in,
                        float* x_out, const int* __restrict__ done) {
    if (finished(done)) return;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        x_out[i] = __fadd_rn(x_in[i], e[aggregate[i]]);
    }
}

// r_i = f_i - (A x)_i, stored for the weighted restriction
template <int LANES>
__global__ __launch_bounds__(kBlock)
void amg_residual_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                         const float* __restrict__ vals, const float* __restrict__ f, const float* __restrict__ x,
                         float* __restrict__ r, const int* __restrict__ done) {
    if (finished(done)) return;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        r[row] = __fsub_rn(f[row], acc);
    });
}

// f_coarse[a] = (PT r)_a: PT's arrays, one lane group per aggregate
template <int LANES>
__global__ __launch_bounds__(kBlock)
void amg_restrict_weighted_kernel(int num_aggregates, long long nnz, const int* __restrict__ row_ptrs,
                                  const int* __restrict__ cols, const float* __restrict__ vals,
                                  const float* __restrict__ r, float* __restrict__ f_coarse,
                                  const int* __restrict__ done) {
    if (finished(done)) return;
    for_each_row_dot<LANES>(num_aggregates, nnz, row_ptrs, cols, vals, r, [&](long long row, float acc) {
        f_coarse[row] = acc;
    });
}

// x_out_i = x_in_i + (P e)_i: P's arrays; x_out may be x_in itself (each element is read and written by one lane)
template <int LANES>
__global__ __launch_bounds__(kBlock)
void amg_prolong_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                        const float* __restrict__ vals, const float* __restrict__ e, const float* x_in, float* x_out,
                        const int* __restrict__ done) {
    if (finished(done)) return;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, e, [&](long long row, float acc) {
        x_out[row] = __fadd_rn(x_in[row], acc);
    });
}

// z_i = sum_j cinv[i * n + j] * f_j: one wavefront per row, lane t takes j = t, t + 64, ... in fp64 (the products
// are exact), the lanes are folded by the xor butterfly 32, 16, ... 1, and the sum is rounded once
__global__ __launch_bounds__(kBlock)
void amg_dense_kernel(int n, const float* __restrict__ cinv, const float* __restrict__ f, float* __restrict__ z,
                      const int* __restrict__ done) {
    if (finished(done)) return;
    constexpr int kWaves = kBlock / 64;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int row = blockIdx.x * kWaves + wave; row < n; row += gridDim.x * kWaves) {
        const float* __restrict__ c = cinv + static_cast<size_t>(row) * n;
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) acc += prod64(c[j], f[j]);
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) z[row] = static_cast<float>(acc);
    }
}

struct Cycle {
    const AMGHierarchy& H;
    const int* done;
    int forced;
    hipStream_t s;

    int lanes_of(const AMGLevel& lv) const { return forced ? forced : lv.lanes; }

    hipError_t scale(const AMGLevel& lv, const float* f, float* x) const {
        const int n = lv.view.num_rows;
        amg_scale_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, lv.d_wd, f, x, done);
        return hipGetLastError();
    }

    hipError_t sweep(const AMGLevel& lv, const float* f, const float* x_in, float* x_out) const {
        const int lanes = lanes_of(lv);
        const CSRMatrix& M = lv.view;
        return with_lanes(lanes, [&](auto L) {
            constexpr int kLanes = decltype(L)::value;
            amg_sweep_kernel<kLanes><<<capped_grid(M.num_rows, kBlock / kLanes), kBlock, 0, s>>>(
                M.num_rows, M.nnz, M.d_row_ptrs, M.d_col_indices, M.d_values, lv.d_wd, f, x_in, x_out, done);
            return hipGetLastError();
        });
    }

    // the row sweep of one of the three kernels below over M: kernel<LANES>(rows, nnz, M's arrays, args..., done)
    template <class Launch>
    hipError_t row_sweep(const CSRMatrix& M, int lanes, Launch&& launch) const {
        return with_lanes(forced ? forced : lanes, [&](auto L) {
            constexpr int kLanes = decltype(L)::value;
            launch(L, capped_grid(M.num_rows, kBlock / kLanes));
            return hipGetLastError();
        });
    }

    hipError_t residual(const AMGLevel& lv, const float* f, const float* x, float* r) const {
        const CSRMatrix& M = lv.view;
        return row_sweep(M, lv.lanes, [&](auto L, int grid) {
            amg_residual_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(
                M.num_rows, M.nnz, M.d_row_ptrs, M.d_col_indices, M.d_values, f, x, r, done);
        });
    }

    hipError_t restrict_weighted(const AMGLevel& lv, const float* r, float* f_coarse) const {
        const CSRMatrix& M = *lv.PT;
        return row_sweep(M, lv.pt_lanes, [&](auto L, int grid) {
            amg_restrict_weighted_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(
                M.num_rows, M.nnz, M.d_row_ptrs, M.d_col_indices, M.d_values, r, f_coarse, done);
        });
    }

    hipError_t prolong(const AMGLevel& lv, const float* e, const float* x_in, float* x_out) const {
        const CSRMatrix& M = *lv.P;
        return row_sweep(M, lv.p_lanes, [&](auto L, int grid) {
            amg_prolong_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(
                M.num_rows, M.nnz, M.d_row_ptrs, M.d_col_indices, M.d_values, e, x_in, x_out, done);
        });
    }

    // f_coarse = the restricted residual of (f, x), by the hierarchy's kind
    hipError_t down(const AMGLevel& lv, const float* f, const float* x, float* f_coarse) const {
        if (!H.smoothed) return restrict_to(lv, f, x, f_coarse);
        const hipError_t e = residual(lv, f, x, lv.d_res);
        return e == hipSuccess ? restrict_weighted(lv, lv.d_res, f_coarse) : e;
    }

    // x_out = x_in + the prolonged e, by the hierarchy's kind
    hipError_t up(const AMGLevel& lv, const float* e, const float* x_in, float* x_out) const {
        return H.smoothed ? prolong(lv, e, x_in, x_out) : correct(lv, e, x_in, x_out);
    }

    hipError_t restrict_to(const AMGLevel& lv, const float* f, const float* x, float* f_coarse) const {
        const int lanes = lanes_of(lv);
        const CSRMatrix& M = lv.view;
        return with_lanes(lanes, [&](auto L) {
            constexpr int kLanes = decltype(L)::value;
            amg_restrict_kernel<kLanes><<<capped_grid(lv.num_aggregates, kBlock / kLanes), kBlock, 0, s>>>(
                lv.num_aggregates, M.nnz, M.d_row_ptrs, M.d_col_indices, M.d_values, lv.PT->d_row_ptrs,
                lv.PT->d_col_indices, f, x, f_coarse, done);
            return hipGetLastError();
        });
    }

    hipError_t correct(const AMGLevel& lv, const float* e, const float* x_in, float* x_out) const {
        const int n = lv.view.num_rows;
        amg_correct_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, lv.P->d_col_indices, e, x_in, x_out, done);
        return hipGetLastError();
    }

    // `count` >= 1 sweeps from a zero guess; write k goes to xa / xb in turn, the last one to `last` when it is given.
    // Returns where the result lies through *where.
    hipError_t sweeps_from_zero(const AMGLevel& lv, const float* f, int count, float* xa, float* xb, float* last,
                                const float** where) const {
        float* cur = (count == 1 && last) ? last : xa;
        hipError_t e = scale(lv, f, cur);
        for (int k = 1; e == hipSuccess && k < count; ++k) {
            float* next = (k == count - 1 && last) ? last : (cur == xa ? xb : xa);
            e = sweep(lv, f, cur, next);
            cur = next;
        }
        *where = cur;
        return e;
    }
};

} // namespace

int amg_forced_lanes() { return forced_lanes("amg_lanes"); }

hipError_t amg_vcycle(const AMGHierarchy& H, const float* d_r, float* d_z, const int* d_done, int forced_lanes,
                      hipStream_t s) {
    const Cycle cycle{H, d_done, forced_lanes, s};
    const int levels = static_cast<int>(H.levels.size());
    const int coarsest = levels - 1;
    // the vectors of a level inside its slab
    const auto f_of = [&](int l) -> const float* { return l == 0 ? d_r : H.levels[l].d_work; };
    const auto out_of = [&](int l) -> float* {
        return l == 0 ? d_z : H.levels[l].d_work + static_cast<size_t>(H.levels[l].view.num_rows);
    };
    const auto xa_of = [&](int l) -> float* {
        return H.levels[l].d_work + (l == 0 ? 0 : 2 * static_cast<size_t>(H.levels[l].view.num_rows));
    };
    const auto xb_of = [&](int l) -> float* { return xa_of(l) + static_cast<size_t>(H.levels[l].view.num_rows); };

    std::vector<const float*> x_at(static_cast<size_t>(levels), nullptr);
    hipError_t e = hipSuccess;
    // down: smooth, then the residual restricted into the next level's right-hand side
    for (int l = 0; e == hipSuccess && l < coarsest; ++l) {
        const AMGLevel& lv = H.levels[l];
        e = cycle.sweeps_from_zero(lv, f_of(l), H.config.pre_sweeps, xa_of(l), xb_of(l), nullptr, &x_at[l]);
        if (e == hipSuccess) e = cycle.down(lv, f_of(l), x_at[l], H.levels[l + 1].d_work);
    }
    if (e != hipSuccess) return e;
    // the coarsest level
    {
        const AMGLevel& lv = H.levels[coarsest];
        const int n = lv.view.num_rows;
        if (H.coarse_solver == 0) {
            constexpr int kWaves = kBlock / 64;
            amg_dense_kernel<<<(n + kWaves - 1) / kWaves, kBlock, 0, s>>>(n, H.d_cinv, f_of(coarsest),
                                                                          out_of(coarsest), d_done);
            e = hipGetLastError();
        } else {
            const float* unused = nullptr;
            e = cycle.sweeps_from_zero(lv, f_of(coarsest), H.config.coarse_sweeps, xa_of(coarsest), xb_of(coarsest),
                                       out_of(coarsest), &unused);
        }
    }
    // up: correct, then smooth; the last write of a level goes to its output vector
    const int post = H.config.post_sweeps;
    for (int l = coarsest - 1; e == hipSuccess && l >= 0; --l) {
        const AMGLevel& lv = H.levels[l];
        const float* err = out_of(l + 1);
        float* cur = const_cast<float*>(x_at[l]);
        if (post == 0) {
            e = cycle.up(lv, err, cur, out_of(l));
            continue;
        }
        e = cycle.up(lv, err, cur, cur);
        for (int k = 0; e == hipSuccess && k < post; ++k) {
            float* next = k == post - 1 ? out_of(l) : (cur == xa_of(l) ? xb_of(l) : xa_of(l));
            e = cycle.sweep(lv, f_of(l), cur, next);
            cur = next;
        }
    }
    return e;
}

} // namespace detail

int amg_apply(const AMGHierarchy* H, const float* d_r, float* d_z) {
    using namespace detail;
    if (!H || !d_r || !d_z || H->levels.empty()) return code(SpMVError::INVALID_ARGUMENT);
    if (solver::ranges_overlap(d_r, d_z, H->num_rows)) return code(SpMVError::INVALID_ARGUMENT);
    const TraceRange range("spmv:amg_apply");
    hipStream_t stream = current_stream();
    if (amg_vcycle(*H, d_r, d_z, nullptr, amg_forced_lanes(), stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}

namespace {

// the checks amg_restrict and amg_prolong share; 0, or an SpMVError code
int transfer_level_checked(const AMGHierarchy* H, int level, bool pointers_ok) {
    using namespace detail;
    if (!H || !pointers_ok || H->levels.empty()) return code(SpMVError::INVALID_ARGUMENT);
    if (level < 0 || level + 1 >= static_cast<int>(H->levels.size())) return code(SpMVError::INVALID_DIMENSION);
    return 0;
}

// [a, a + na) and [b, b + nb) floats share a byte
bool floats_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) && b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

int transfer_finished(hipError_t e, hipStream_t stream) {
    using namespace detail;
    if (e != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}

} // namespace

int amg_restrict(const AMGHierarchy* H, int level, const float* d_f, const float* d_x, float* d_f_coarse) {
    using namespace detail;
    if (const int status = transfer_level_checked(H, level, d_f && d_x && d_f_coarse)) return status;
    const AMGLevel& lv = H->levels[static_cast<size_t>(level)];
    const long long n = lv.view.num_rows, nc = lv.num_aggregates;
    if (floats_overlap(d_f_coarse, nc, d_f, n) || floats_overlap(d_f_coarse, nc, d_x, n)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const TraceRange range("spmv:amg_restrict");
    hipStream_t stream = current_stream();
    const Cycle cycle{*H, nullptr, amg_forced_lanes(), stream};
    return transfer_finished(cycle.down(lv, d_f, d_x, d_f_coarse), stream);
}

int amg_prolong(const AMGHierarchy* H, int level, const float* d_e, float* d_x) {
    using namespace detail;
    if (const int status = transfer_level_checked(H, level, d_e && d_x)) return status;
    const AMGLevel& lv = H->levels[static_cast<size_t>(level)];
    if (floats_overlap(d_e, lv.num_aggregates, d_x, lv.view.num_rows)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const TraceRange range("spmv:amg_prolong");
    hipStream_t stream = current_stream();
    const Cycle cycle{*H, nullptr, amg_forced_lanes(), stream};
    return transfer_finished(cycle.up(lv, d_e, d_x, d_x), stream);
}

} // namespace spmv
