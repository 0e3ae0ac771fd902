// gmres.hip — device-resident restarted GMRES(m) (include/spmv/gmres.h).
//
// Built like bicgstab.hip: the Hessenberg column, the rotations and the stop tests live in device memory, every
// gated kernel returns at once when the state says so, and the host reads a two-deep pinned mirror of the state so
// that it enqueues step k+1 before it looks at the outcome of step k.  The state has two phases: `open` (a cycle
// accepts Arnoldi steps) and closed (the cycle waits for its close sequence); step kernels run only while open,
// close kernels only while closed, so either sequence enqueued at the wrong moment changes nothing.
//
// A step, column j (the basis vectors v_0..v_j are ready, with JACOBI also z = v_j * dinv):
//   [LU: z = U^-1 (L^-1 v_j), TriangularPair::apply's two launch_sptrsv sequences]
//   gmres_spmv<LANES> / tiled_spmv    w = A z
//   gmres_multidot                    one pass over w and v_0..v_j: (j+1) partials per workgroup of h1_i = v_i.w
//   gmres_update_multidot             folds h1, w -= h1_i v_i, then the partials of h2_i = v_i.w on the updated w
//   gmres_update_norm                 folds h2, w -= h2_i v_i, and the partials of w.w
//   gmres_hessenberg (one workgroup)  folds w.w; rotations, stop tests, commits the column; 1 / h_j+1 for the scale
//   gmres_normalize                   v_j+1 = w * scale (JACOBI: z = v_j+1 * dinv)
// The close sequence of a cycle with k columns (setup is the same sequence with k = 0):
//   gmres_backsub (one workgroup)     R y = g in fp64, y rounded to fp32
//   gmres_correct                     u = sum y_i v_i; x += u (NONE), x += u * dinv (JACOBI), u stored (LU)
//   [LU: z = U^-1 (L^-1 u), then gmres_add: x += z]
//   gmres_residual<LANES>             r = b - A x into w, partials of r.r and b.b
//     (tiled: tiled_spmv into the u buffer, then gmres_residual_ew)
//   gmres_begin (one workgroup)       folds them: converged / done, or opens the next cycle: g_0 = beta, 1 / beta
//   gmres_normalize                   v_0 = w * scale (only right after gmres_begin opened a cycle: k == 0)
// A one-workgroup kernel is the only writer of the state, and no kernel reads a state field that a kernel of the
// same launch writes.  The ungated launches (tiled_spmv, launch_sptrsv) write only w, u or z, which hold nothing
// live at a step boundary.
//
// The host side is built from solver_common.h's parts (Workspace and its mirror, TriangularPair, TiledEngine,
// diag_kernel); what is here is this solver's checks, its workspace layout, its launches, the cycle bookkeeping
// and its result.
//
// The three orthogonalisation kernels are made of basis_ops.h's functions (shared with eigs.hip): they walk the basis
// in compile-time groups of kGroup vectors with kGroup fp64 accumulators in registers.
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"
#include "basis_ops.h"
#include "tiled.h"
#include "spmv/gmres.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;
using namespace basis;

constexpr int kMaxRestart = 64;

// Lives in device memory and is mirrored to the host after every step.
struct GmresState {
    double bnorm;             // ||b||_2
    double threshold;         // tolerance * ||b||_2
    float  scale;             // 1 / beta (gmres_begin) or 1 / h_j+1 (gmres_hessenberg): what gmres_normalize applies
    float  relative_residual; // ||b - A x|| / ||b|| as last recomputed
    int    iterations;        // committed columns over all cycles
    int    cycles;            // cycles opened
    int    k;                 // committed columns of this cycle
    int    open;              // 1: the cycle accepts steps; 0: it waits for its close sequence
    int    final_cycle;       // the close in flight ends the solve (max_iterations reached or a breakdown)
    int    converged;
    int    breakdown;         // GMRESResult::Breakdown
    int    done;              // everything after this is a no-op
    int    zero_b;            // ||b|| == 0: the host writes x = 0
    int    bad_diagonal;      // JACOBI / LU: some row's diagonal is missing, zero or not finite
};

// fp64 work arrays of the small problem, in one allocation
struct Small {
    double* R;       // kMaxRestart columns of kMaxRestart: R[j * kMaxRestart + i], i <= j
    double* g;       // kMaxRestart + 1
    double* cs;      // kMaxRestart
    double* sn;      // kMaxRestart
    float*  h1;      // fp32(h1_i) of this step (gmres_update_multidot, workgroup 0)
    float*  h2;      // fp32(h2_i) of this step (gmres_update_norm, workgroup 0)
    float*  y;       // fp32(y_i) of this close (gmres_backsub)
};
constexpr size_t kSmallDoubles = kMaxRestart * kMaxRestart + (kMaxRestart + 8) + 2 * kMaxRestart +
                                 (3 * kMaxRestart * sizeof(float)) / sizeof(double);

__device__ __forceinline__ bool stepping(const GmresState* st) { return st->open && !st->done; }
__device__ __forceinline__ bool closing(const GmresState* st) { return !st->open && !st->done; }

__global__ __launch_bounds__(kBlock)
void gmres_multidot(long long n, long long ld, int j, const float* __restrict__ V, const float* __restrict__ w,
                    const GmresState* __restrict__ st, double* __restrict__ part1) {
    if (!stepping(st)) return;
    multidot_pass(n, ld, j + 1, V, w, part1);
}

__global__ __launch_bounds__(kBlock)
void gmres_update_multidot(long long n, long long ld, int j, const float* __restrict__ V, float* w,
                           const GmresState* __restrict__ st, const double* __restrict__ part1,
                           float* __restrict__ h1, double* __restrict__ part2) {
    if (!stepping(st)) return;
    __shared__ float s_h[kMaxRestart];
    const int nv = j + 1;
    fold_columns(part1, gridDim.x, nv, s_h);
    if (blockIdx.x == 0 && threadIdx.x < nv) h1[threadIdx.x] = s_h[threadIdx.x];
    for (long long base = static_cast<long long>(blockIdx.x) * kChunk; base < n;
         base += static_cast<long long>(gridDim.x) * kChunk) {
        const long long e = base + 4 * threadIdx.x;
        store4(w, e, n, subtract_all(n, ld, nv, V, s_h, e, load4_masked(w, e, n)));
    }
    multidot_pass(n, ld, nv, V, w, part2);      // each thread reads back the elements it wrote itself
}

__global__ __launch_bounds__(kBlock)
void gmres_update_norm(long long n, long long ld, int j, const float* __restrict__ V, float* w,
                       const GmresState* __restrict__ st, const double* __restrict__ part2,
                       float* __restrict__ h2, double* __restrict__ ww_part) {
    if (!stepping(st)) return;
    __shared__ float s_h[kMaxRestart];
    const int nv = j + 1;
    fold_columns(part2, gridDim.x, nv, s_h);
    if (blockIdx.x == 0 && threadIdx.x < nv) h2[threadIdx.x] = s_h[threadIdx.x];
    double ww = 0.0, unused = 0.0;
    for (long long base = static_cast<long long>(blockIdx.x) * kChunk; base < n;
         base += static_cast<long long>(gridDim.x) * kChunk) {
        const long long e = base + 4 * threadIdx.x;
        const f32x4 w4 = subtract_all(n, ld, nv, V, s_h, e, load4_masked(w, e, n));
        store4(w, e, n, w4);
        ww += dot4(w4, w4);
    }
    block_sum2(ww, unused);
    if (threadIdx.x == 0) ww_part[blockIdx.x] = ww;
}

// One workgroup.  Column j: h_i = double(fp32 h1_i) + double(fp32 h2_i), h_j+1 = sqrt(w.w); the earlier rotations,
// the new one, g; the stop tests; commits the column and closes the cycle, or leaves 1 / h_j+1 for gmres_normalize.
__global__ __launch_bounds__(kBlock)
void gmres_hessenberg(int j, int restart, int max_iterations, const double* __restrict__ ww_part, int ww_count,
                      Small sm, GmresState* __restrict__ st) {
    if (!stepping(st)) return;
    __shared__ double s_col[kMaxRestart + 1];
    double ww = 0.0, unused = 0.0;
    fold_partials(ww_part, ww_count, 1, ww, unused);
    if (threadIdx.x <= j) {
        s_col[threadIdx.x] = static_cast<double>(sm.h1[threadIdx.x]) + static_cast<double>(sm.h2[threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double hn = sqrt(ww);
    for (int i = 0; i < j; ++i) {
        const double a = s_col[i], b = s_col[i + 1], c = sm.cs[i], s = sm.sn[i];
        s_col[i] = __dadd_rn(__dmul_rn(c, a), __dmul_rn(s, b));
        s_col[i + 1] = __dadd_rn(__dmul_rn(-s, a), __dmul_rn(c, b));
    }
    bool finite = isfinite(hn);
    for (int i = 0; i <= j; ++i) finite = finite && isfinite(s_col[i]);
    const double a = s_col[j];
    const double d = sqrt(__dadd_rn(__dmul_rn(a, a), __dmul_rn(hn, hn)));
    finite = finite && isfinite(d);
    if (!finite || d == 0.0) {                  // column j is not committed: the close applies columns 0..j-1
        st->breakdown = finite ? GMRESResult::SINGULAR : GMRESResult::NOT_FINITE;
        st->k = j;
        st->final_cycle = 1;
        st->open = 0;
        return;
    }
    const double c = a / d, s = hn / d;
    sm.cs[j] = c;
    sm.sn[j] = s;
    s_col[j] = d;
    for (int i = 0; i <= j; ++i) sm.R[j * kMaxRestart + i] = s_col[i];
    const double gj = sm.g[j];
    const double gnext = __dmul_rn(-s, gj);
    sm.g[j + 1] = gnext;
    sm.g[j] = __dmul_rn(c, gj);
    const int total = st->iterations + 1;
    st->iterations = total;
    st->k = j + 1;
    if (total >= max_iterations) st->final_cycle = 1;
    if (fabs(gnext) <= st->threshold || j + 1 == restart || total >= max_iterations || hn == 0.0) {
        st->open = 0;
    } else {
        st->scale = static_cast<float>(1.0 / hn);
    }
}

// dst = w * scale; with JACOBI also z = dst * dinv.  `at_begin`: the v_0 of a cycle gmres_begin has just opened
// (k == 0), else the v_j+1 of a step that left the cycle open.
__global__ __launch_bounds__(kBlock)
void gmres_normalize(long long n, int at_begin, const float* __restrict__ w, float* __restrict__ dst,
                     const float* __restrict__ dinv, float* __restrict__ z, const GmresState* __restrict__ st) {
    if (!stepping(st) || (at_begin && st->k != 0)) return;
    const float scale = st->scale;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float vi = __fmul_rn(w[i], scale);
        dst[i] = vi;
        if (dinv) z[i] = __fmul_rn(vi, dinv[i]);
    }
}

// One workgroup: R y = g over the k committed columns, fp64, every product and sum rounded; y rounded to fp32.
__global__ __launch_bounds__(kBlock)
void gmres_backsub(Small sm, const GmresState* __restrict__ st) {
    if (!closing(st)) return;
    __shared__ double s_y[kMaxRestart];
    const int k = st->k;
    if (threadIdx.x != 0) return;
    for (int i = k - 1; i >= 0; --i) {
        double s = sm.g[i];
        for (int l = i + 1; l < k; ++l) s = __dadd_rn(s, -__dmul_rn(sm.R[l * kMaxRestart + i], s_y[l]));
        const double yi = s / sm.R[i * kMaxRestart + i];
        s_y[i] = yi;
        sm.y[i] = static_cast<float>(yi);
    }
}

// u = sum over i < k ascending of fmaf(y_i, v_i, u) from 0.  mode 0 (NONE): x += u; 1 (JACOBI): x += u * dinv;
// 2 (LU): u is stored for the triangular solves.  x may be misaligned: scalar accesses.
__global__ __launch_bounds__(kBlock)
void gmres_correct(long long n, long long ld, int mode, const float* __restrict__ V, const float* __restrict__ y,
                   const float* __restrict__ dinv, float* __restrict__ u, float* __restrict__ x,
                   const GmresState* __restrict__ st) {
    if (!closing(st)) return;
    const int k = st->k;
    if (k == 0) return;
    __shared__ float s_y[kMaxRestart];
    if (threadIdx.x < k) s_y[threadIdx.x] = y[threadIdx.x];
    __syncthreads();
    for (long long base = static_cast<long long>(blockIdx.x) * kChunk; base < n;
         base += static_cast<long long>(gridDim.x) * kChunk) {
        const long long e = base + 4 * threadIdx.x;
        f32x4 u4 = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int first = 0; first < k; first += kGroup) {
            const int count = min(kGroup, k - first);
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                if (i < count) {
                    const float yi = s_y[first + i];
                    const f32x4 v4 = load4_masked(V + (first + i) * ld, e, n);
#pragma unroll
                    for (int q = 0; q < 4; ++q) u4[q] = __builtin_fmaf(yi, v4[q], u4[q]);
                }
            }
        }
        if (mode == 2) {
            store4(u, e, n, u4);
        } else {
            const f32x4 d4 = mode == 1 ? load4_masked(dinv, e, n) : u4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (e + q < n) x[e + q] = __fadd_rn(x[e + q], mode == 1 ? __fmul_rn(u4[q], d4[q]) : u4[q]);
            }
        }
    }
}

// LU: x += z, z = U^-1 (L^-1 u)
__global__ __launch_bounds__(kBlock)
void gmres_add(long long n, const float* __restrict__ z, float* __restrict__ x, const GmresState* __restrict__ st) {
    if (!closing(st) || st->k == 0) return;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        x[i] = __fadd_rn(x[i], z[i]);
    }
}

// r = b - A x into `r` and the block partials of r.r and b.b -> part[2 * block]
template <int LANES>
__global__ __launch_bounds__(kBlock)
void gmres_residual(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                    const float* __restrict__ vals, const float* __restrict__ b, const float* __restrict__ x,
                    float* __restrict__ r, const GmresState* __restrict__ st, double* __restrict__ part) {
    if (!closing(st)) return;
    double rr = 0.0, bb = 0.0;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, x, [&](long long row, float acc) {
        const float bi = b[row];
        const float ri = __fsub_rn(bi, acc);
        r[row] = ri;
        rr += prod64(ri, ri);
        bb += prod64(bi, bi);
    });
    block_sum2(rr, bb);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = rr;
        part[2 * blockIdx.x + 1] = bb;
    }
}

// the same with A x given (tiled engine)
__global__ __launch_bounds__(kBlock)
void gmres_residual_ew(long long n, const float* __restrict__ b, const float* __restrict__ ax, float* __restrict__ r,
                       const GmresState* __restrict__ st, double* __restrict__ part) {
    if (!closing(st)) return;
    double rr = 0.0, bb = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float bi = b[i];
        const float ri = __fsub_rn(bi, ax[i]);
        r[i] = ri;
        rr += prod64(ri, ri);
        bb += prod64(bi, bi);
    }
    block_sum2(rr, bb);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = rr;
        part[2 * blockIdx.x + 1] = bb;
    }
}

// One workgroup: folds r.r and b.b.  Ends the solve (converged, not finite, or the closed cycle was the last one)
// or opens the next cycle: g_0 = beta, scale = fp32(1 / beta).
__global__ __launch_bounds__(kBlock)
void gmres_begin(const double* __restrict__ part, int count, float tolerance, int max_iterations, Small sm,
                 GmresState* __restrict__ st) {
    if (!closing(st)) return;
    double rr = 0.0, bb = 0.0;
    fold_partials(part, count, 2, rr, bb);
    if (threadIdx.x != 0) return;
    const double bnorm = sqrt(bb);
    const double beta = sqrt(rr);
    const double threshold = static_cast<double>(tolerance) * bnorm;
    st->bnorm = bnorm;
    st->threshold = threshold;
    if (bb == 0.0) {
        st->zero_b = 1;
        st->relative_residual = 0.0f;
        st->converged = 1;
        st->done = 1;
        return;
    }
    st->relative_residual = static_cast<float>(beta / bnorm);
    if (!isfinite(bb) || !isfinite(rr)) {
        if (st->breakdown == GMRESResult::NONE) st->breakdown = GMRESResult::NOT_FINITE;
        st->done = 1;
    } else if (beta <= threshold) {
        st->converged = 1;
        st->done = 1;
    } else if (st->final_cycle || st->iterations >= max_iterations) {
        st->done = 1;
    } else {
        sm.g[0] = beta;
        st->scale = static_cast<float>(1.0 / beta);
        st->k = 0;
        st->cycles += 1;
        st->open = 1;
    }
}

// w = A v (vector CSR), while a cycle is open
template <int LANES>
__global__ __launch_bounds__(kBlock)
void gmres_spmv(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                const float* __restrict__ vals, const float* __restrict__ v, float* __restrict__ w,
                const GmresState* __restrict__ st) {
    if (!stepping(st)) return;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, v, [&](long long row, float sum) { w[row] = sum; });
}

// gmres_solve (with_lu false: cfg.preconditioner picks NONE or JACOBI) and gmres_solve_lu (with_lu true: M = L U
// from LU, cfg.preconditioner is not read).
GMRESResult solve(const CSRMatrix* A, const CSRMatrix* LU, bool with_lu, const float* d_b, float* d_x,
                  const GMRESConfig* config) {
    GMRESResult result;
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
    const GMRESConfig defaults;
    const GMRESConfig& cfg = config ? *config : defaults;
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 || cfg.restart < 1 || cfg.restart > kMaxRestart ||
        (!with_lu && cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI) ||
        cfg.engine < -1 || cfg.engine > 1) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const int n = A->num_rows;
    if (ranges_overlap(d_b, d_x, n)) return fail(SpMVError::INVALID_ARGUMENT);

    const TraceRange range(with_lu ? "spmv:gmres_solve_lu" : "spmv:gmres_solve");
    hipStream_t stream = current_stream();
    const bool jacobi = !with_lu && cfg.preconditioner == CGConfig::JACOBI;
    const int mode = with_lu ? 2 : jacobi ? 1 : 0;
    const int restart = cfg.restart;
    const int max_it = cfg.max_iterations;

    TriangularPair lu;              // M = L U: L's diagonal is the implied 1
    if (with_lu) {
        const int status = lu.build(LU, 1, stream);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }
    TiledEngine engine(A, cfg.engine, stream);

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const int ogrid = static_cast<int>(std::min<long long>((static_cast<long long>(n) + kChunk - 1) / kChunk,
                                                           kOrthoBlocks));
    // the basis: restart + 1 vectors, leading dimension a multiple of 256 bytes; then w, u and, when M != I, z;
    // with JACOBI dinv.  Every vector starts on a 256-byte boundary.
    const size_t ld = (static_cast<size_t>(n) + 63) / 64 * 64;
    const size_t basis = static_cast<size_t>(restart + 1) * ld;
    const size_t res_count = 2 * static_cast<size_t>(std::max(row_grid, vgrid));
    const size_t col_count = static_cast<size_t>(kMaxRestart) * ogrid;
    Workspace<GmresState> ws;
    if (!ws.allocate(basis + (mode == 1 ? 4 : mode == 2 ? 3 : 2) * ld,
                     2 * col_count + ogrid + res_count + kSmallDoubles)) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    float* V = ws.vec;
    float* w = V + basis;
    float* u = w + ld;
    float* z = mode != 0 ? u + ld : nullptr;
    float* dinv = mode == 1 ? z + ld : nullptr;
    double* part1 = ws.part;
    double* part2 = part1 + col_count;
    double* ww_part = part2 + col_count;
    double* res_part = ww_part + ogrid;
    Small sm;
    sm.R = res_part + res_count;
    sm.g = sm.R + kMaxRestart * kMaxRestart;
    sm.cs = sm.g + kMaxRestart + 8;
    sm.sn = sm.cs + kMaxRestart;
    sm.h1 = reinterpret_cast<float*>(sm.sn + kMaxRestart);
    sm.h2 = sm.h1 + kMaxRestart;
    sm.y = sm.h2 + kMaxRestart;
    float* z_out = jacobi ? z : nullptr;           // gmres_normalize writes z only with JACOBI

    // r = b - A x into w, its partials, gmres_begin, v_0: the tail of every close sequence, and the setup
    const auto residual_and_begin = [&]() -> bool {
        int count = row_grid;
        const TiledEngine::Spmv spmv = engine.spmv(d_x, u, stream);
        if (spmv == TiledEngine::Spmv::FAILED) return false;
        if (spmv == TiledEngine::Spmv::TILED) {
            gmres_residual_ew<<<vgrid, kBlock, 0, stream>>>(n, d_b, u, w, ws.state, res_part);
            count = vgrid;
        } else {
            const hipError_t e = with_lanes(lanes, [&](auto L) {
                gmres_residual<decltype(L)::value><<<row_grid, kBlock, 0, stream>>>(
                    n, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, d_b, d_x, w, ws.state, res_part);
                return hipGetLastError();
            });
            if (e != hipSuccess) return false;
        }
        gmres_begin<<<1, kBlock, 0, stream>>>(res_part, count, cfg.tolerance, max_it, sm, ws.state);
        gmres_normalize<<<vgrid, kBlock, 0, stream>>>(n, 1, w, V, dinv, z_out, ws.state);
        return hipGetLastError() == hipSuccess;
    };
    const auto close_cycle = [&]() -> bool {
        gmres_backsub<<<1, kBlock, 0, stream>>>(sm, ws.state);
        gmres_correct<<<ogrid, kBlock, 0, stream>>>(n, static_cast<long long>(ld), mode, V, sm.y, dinv, u, d_x,
                                                    ws.state);
        if (hipGetLastError() != hipSuccess) return false;
        if (with_lu) {
            if (!lu.apply(u, z, stream)) return false;
            gmres_add<<<vgrid, kBlock, 0, stream>>>(n, z, d_x, ws.state);
        }
        return residual_and_begin();
    };
    const auto step = [&](int j) -> bool {
        const float* vj = V + static_cast<size_t>(j) * ld;
        if (with_lu && !lu.apply(vj, z, stream)) return false;
        const float* in = mode == 0 ? vj : z;
        const TiledEngine::Spmv spmv = engine.spmv(in, w, stream);
        if (spmv == TiledEngine::Spmv::FAILED) return false;
        if (spmv == TiledEngine::Spmv::DIRECT) {
            const hipError_t e = with_lanes(lanes, [&](auto L) {
                gmres_spmv<decltype(L)::value><<<row_grid, kBlock, 0, stream>>>(
                    n, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, in, w, ws.state);
                return hipGetLastError();
            });
            if (e != hipSuccess) return false;
        }
        const long long lld = static_cast<long long>(ld);
        gmres_multidot<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part1);
        gmres_update_multidot<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part1, sm.h1, part2);
        gmres_update_norm<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part2, sm.h2, ww_part);
        gmres_hessenberg<<<1, kBlock, 0, stream>>>(j, restart, max_it, ww_part, ogrid, sm, ws.state);
        gmres_normalize<<<vgrid, kBlock, 0, stream>>>(n, 0, w, V + static_cast<size_t>(j + 1) * ld, dinv, z_out,
                                                      ws.state);
        return hipGetLastError() == hipSuccess;
    };

    // setup: the diagonal (JACOBI; of LU only its check), then the close sequence of a cycle without columns; one
    // read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(GmresState), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (with_lu) ok = ok && launch_diag<DiagRule::NONZERO_FINITE>(LU, nullptr, bad, stream) == hipSuccess;
    if (jacobi) ok = ok && launch_diag<DiagRule::NONZERO_FINITE>(A, dinv, bad, stream) == hipSuccess;
    if (!ws.read_back(ok && residual_and_begin(), stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (ws.pinned[0].bad_diagonal) return fail(SpMVError::INVALID_ARGUMENT);
    if (ws.pinned[0].zero_b) {
        if (!zero_solution(d_x, static_cast<size_t>(n), stream)) return fail(SpMVError::KERNEL_LAUNCH);
        result.converged = 1;
        return result;
    }

    if (!ws.pinned[0].done) {
        EventPair& ev = thread_events();
        ok = hipEventRecord(ev.start, stream) == hipSuccess;
        // The host follows the device's column j and step count: a cycle that closes where the host expects it
        // (j + 1 == restart, the step count reaches max_iterations) gets its close sequence at once.  One that
        // closes early shows in the mirror one step late: the step enqueued in between was a no-op, the close
        // follows now and the host's counters are set from the mirror.  Every cycle but a broken one commits a
        // column, so 2 * max_iterations + 2 steps bound the loop.
        int j = 0;
        long long steps = 0;
        const long long bound = 2LL * max_it + 2;
        for (long long it = 0; ok && it < bound; ++it) {
            if (!engine.build_if_due(it, ws, stream, ok)) break;
            const TraceRange step_range("spmv:gmres_step");
            ok = ok && step(j);
            ++steps;
            const bool closed_here = j + 1 == restart || steps >= max_it;
            if (ok && closed_here) ok = close_cycle();
            j = closed_here ? 0 : j + 1;
            if (ok && it >= 1) {
                const GmresState* seen = ws.wait_previous(it);
                ok = seen != nullptr;
                if (ok && seen->done) break;
                if (ok && !seen->open) {            // closed early at step it - 1: step `it` did nothing
                    if (!closed_here) ok = close_cycle();
                    j = 0;
                    steps = seen->iterations;
                }
            }
            ok = ok && ws.publish(it, sizeof(GmresState), stream);
        }
        if (!ws.finish_timed(ok, ev, stream, &result.elapsed_ms)) return fail(SpMVError::KERNEL_LAUNCH);
    }
    const GmresState& final_state = ws.pinned[0];
    result.iterations = final_state.iterations;
    result.restarts = std::max(final_state.cycles - 1, 0);
    result.relative_residual = final_state.relative_residual;
    result.converged = final_state.converged;
    result.breakdown = final_state.breakdown;
    return result;
}

} // namespace
} // namespace detail

GMRESResult gmres_solve(const CSRMatrix* A, const float* d_b, float* d_x, const GMRESConfig* config) {
    return detail::solve(A, nullptr, false, d_b, d_x, config);
}

GMRESResult gmres_solve_lu(const CSRMatrix* A, const CSRMatrix* LU, const float* d_b, float* d_x,
                           const GMRESConfig* config) {
    return detail::solve(A, LU, true, d_b, d_x, config);
}

} // namespace spmv
