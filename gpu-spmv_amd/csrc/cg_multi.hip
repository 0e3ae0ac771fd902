// cg_multi.hip — cg_solve for k right-hand sides in one matrix pass per step (include/spmv/cg.h cg_solve_multi,
// DESIGN.md §4.17).
//
// cg.hip's direct-engine loop, k-wide: B and X are num_rows x k row-major; r, p and q live in a workspace cut into
// windows of W = 4 (k <= 4) or 8 columns, each window a num_rows x W row-major array of its own (so a pass over one
// window streams whole lines and every row slice is 16-byte aligned); every column has its own device state
// (CgColumn) and its own partials, and a header in front of the column states carries the global `done` the host
// polls.  Per step, three launches whatever k:
//   cgm_spmv_dot<LANES, W, NW>  Q = A P and, per column, the block partials of p.q
//   cgm_update_kernel<W, false>     per column: the fold of p.q, alpha, x += alpha p, r -= alpha q, partials of r.z, r.r
//   cgm_direction_kernel<W, false>  per column: the fold, beta and the stop test, p = z + beta p; workgroup 0 commits
// Column j is bit for bit cg_solve(engine = 0) on that column: a row's sum is row_partial_dot<LANES>'s walk with one
// accumulator per column, the thread-to-row mapping and the grids are cg.hip's, a thread of the element-wise
// kernels owns row i of the k-wide vectors where cg.hip's owns element i, and each column's partials are laid out
// and folded as cg.hip lays out and folds its own.  A column that is done is frozen: no kernel writes its x, r, p
// or state again.  No float atomics, no waiting between workgroups.
//
// cg_solve_multi_ic is cg.hip's stored-z loop, k-wide: Z is a fourth windowed array, the SpMV half
// of a step is cgm_spmv_dot unchanged, and the second half is
//   cgm_update_kernel<W, true>     the same kernel with STORED_Z: only the partials of r.r (z does not exist yet)
//   TriangularPair::apply          Z = L^-1 R (LOWER NON_UNIT), then Z = L^-T Z in place (UPPER NON_UNIT): ONE k-wide
//                                  launch sequence each (sptrsv_multi.hip on the windowed workspace, no copy)
//   cgm_rz_kernel<W>               per column the partials of r.z
//   cgm_direction_kernel<W, true>  the same kernel with z read from memory
// so a step has cg_solve_ic's launches whatever k.  The triangular solves do not read `done`, as cg.hip's do not: they
// recompute Z for all k columns (the padding columns of the last window included) from an R that no longer changes
// for a frozen column.  A frozen column's Z is never read: cgm_rz_kernel and cgm_direction_kernel skip it.
//
// The host side is built from solver_common.h's parts (Workspace and its mirror, TriangularPair, diag_kernel) and
// multi_window.h's with_window; the k-wide row sum and workgroup reductions are multi_window.h's too.  There is no
// tiled engine here.
#include "internal.h"
#include "device_common.h"
#include "multi_window.h"
#include "solver_common.h"
#include "spmv/cg.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

constexpr int kMaxColumns = 32;

// cg.hip's CgState, one per column.  rz is double-buffered by step parity as there.
struct CgColumn {
    double rz[2];
    double bnorm;
    double threshold;
    float  relative_residual;
    int    iterations;
    int    converged;
    int    breakdown;
    int    done;              // frozen: nothing of this column is written again
    int    zero_b;            // ||b_j|| == 0: column j of X is set to 0
    int    reserved[2];
};

struct CgMultiState {
    int done;                 // every column is done: steps after this are no-ops
    int bad_diagonal;         // JACOBI: some row's diagonal is missing or not > 0
    int reserved[2];
    CgColumn col[kMaxColumns];
};

constexpr size_t kHeaderBytes = offsetof(CgMultiState, col);

// R0 = B - A X0, P0 = Z0 = R0 * dinv, and per column the block partials of r.z, r.r and b.b ->
// part[(3 * gridDim.x) * column + 3 * block].  A window of W columns of B and X at a time (setup: the matrix is
// walked once per window); R and P go into the workspace's windows of WS columns.
template <int LANES, int W, int WS>
__global__ __launch_bounds__(kBlock)
void cgm_init_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                     const float* __restrict__ vals, const float* __restrict__ B, long long ldb,
                     const float* __restrict__ X, long long ldx, bool x_vec, int k,
                     const float* __restrict__ dinv, float* __restrict__ r, float* __restrict__ p,
                     double* __restrict__ part) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    const long long col_stride = 3LL * gridDim.x;
    for (int j0 = 0; j0 < k; j0 += W) {
        const int w = min(W, k - j0);
        // these W columns inside the workspace: window j0 / WS, from its column j0 % WS on
        const long long own = static_cast<long long>(j0 / WS) * n * WS + j0 % WS;
        float* rw = r + own;
        float* pw = p + own;
        double sums[3 * W];           // r.z, r.r, b.b of column j0 + q at [3 * q ..]
#pragma unroll
        for (int q = 0; q < 3 * W; ++q) sums[q] = 0.0;
        for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < n;
             first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
            const long long row = first + slot;
            float acc[W];
#pragma unroll
            for (int q = 0; q < W; ++q) acc[q] = 0.0f;
            if (row < n) {
                row_partial_dot_multi<LANES, W, false>(row_ptrs[row], row_ptrs[row + 1], lane, nnz, cols, vals, X, ldx, j0,
                                                k, x_vec, acc);
            }
#pragma unroll
            for (int q = 0; q < W; ++q) acc[q] = group_sum<LANES>(acc[q]);
            if (lane == 0 && row < n) {
                const float di = dinv ? dinv[row] : 1.0f;
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    if (q < w) {
                        const float bi = B[row * ldb + j0 + q];
                        const float ri = __fsub_rn(bi, acc[q]);
                        const float zi = dinv ? __fmul_rn(ri, di) : ri;
                        rw[row * WS + q] = ri;
                        pw[row * WS + q] = zi;
                        sums[3 * q] += prod64(ri, zi);
                        sums[3 * q + 1] += prod64(ri, ri);
                        sums[3 * q + 2] += prod64(bi, bi);
                    }
                }
            }
        }
        const double total = block_sum_columns<3 * W>(sums);
        if (threadIdx.x < 3 * w) part[col_stride * (j0 + threadIdx.x / 3) + 3LL * blockIdx.x + threadIdx.x % 3] = total;
    }
}

// One workgroup: cg.hip's cg_start_kernel per column, then the global flag.
__global__ __launch_bounds__(kBlock)
void cgm_start_kernel(const double* __restrict__ part, int count, int k, float tolerance,
                      CgMultiState* __restrict__ state) {
    int finished = 0;
    for (int j = 0; j < k; ++j) {
        const double* mine = part + 3LL * count * j;
        double rz = 0.0, rr = 0.0, bb = 0.0, unused = 0.0;
        fold_partials(mine, count, 3, rz, rr);
        fold_partials(mine + 2, count, 3, bb, unused, false);
        if (threadIdx.x != 0) continue;
        CgColumn& c = state->col[j];
        const double bnorm = sqrt(bb);
        const double res = sqrt(rr);
        c.rz[0] = rz;
        c.bnorm = bnorm;
        c.threshold = static_cast<double>(tolerance) * bnorm;
        c.iterations = 0;
        if (bb == 0.0) {
            c.zero_b = 1;
            c.relative_residual = 0.0f;
            c.converged = 1;
            c.done = 1;
        } else {
            c.relative_residual = static_cast<float>(res / bnorm);
            if (res <= c.threshold) {
                c.converged = 1;
                c.done = 1;
            } else if (!(rz > 0.0)) {
                c.breakdown = 1;
                c.done = 1;
            }
        }
        finished += c.done;
    }
    if (threadIdx.x == 0 && finished == k) state->done = 1;
}

// X[:, j] = 0 for every column with ||b_j|| == 0; padding columns are not touched.
__global__ __launch_bounds__(kBlock)
void cgm_zero_kernel(int n, int k, float* __restrict__ X, long long ldx, const CgMultiState* __restrict__ state) {
    const long long total = static_cast<long long>(n) * k;
    for (long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; idx < total;
         idx += static_cast<long long>(gridDim.x) * kBlock) {
        const int j = static_cast<int>(idx % k);
        if (state->col[j].zero_b) X[(idx / k) * ldx + j] = 0.0f;
    }
}

// The columns still running (bit j), the same in every thread of the workgroup: thread 0 reads the flags once and
// LDS hands them round.  0 once the global flag is up.  A workgroup-wide view matters because the folds below hold
// barriers and workgroup 0 raises flags while other workgroups of the same launch are still starting; a workgroup
// that misses a flag raised in its own launch folds the same partials and reaches the same verdict.
__device__ __forceinline__ unsigned active_columns(const CgMultiState* state, int k) {
    __shared__ unsigned s_active;
    if (threadIdx.x == 0) {
        unsigned a = 0;
        if (!state->done) {
            for (int j = 0; j < k; ++j) a |= state->col[j].done ? 0u : 1u << j;
        }
        s_active = a;
    }
    __syncthreads();
    return s_active;
}

// Q = A P and per column the block partials of p.q -> part[part_stride * column + block].  NW windows of W columns
// inside the row loop: the row's entries come from cache after the first window.  A window of frozen columns is
// not walked, and no partial of a frozen column is written.
template <int LANES, int W, int NW>
__global__ __launch_bounds__(kBlock)
void cgm_spmv_dot(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                  const float* __restrict__ vals, const float* __restrict__ p, float* __restrict__ q, int k,
                  const CgMultiState* __restrict__ state, double* __restrict__ part, long long part_stride) {
    const unsigned active = active_columns(state, k);
    if (!active) return;
    constexpr int kRowsPerBlock = kBlock / LANES;
    constexpr unsigned kWindowMask = (1u << W) - 1u;
    const long long window = static_cast<long long>(n) * W;      // floats of one window of the workspace
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    double pq[NW * W];
#pragma unroll
    for (int c = 0; c < NW * W; ++c) pq[c] = 0.0;
    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < n;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long row = first + slot;
        const int begin = row < n ? row_ptrs[row] : 0;
        const int end = row < n ? row_ptrs[row + 1] : 0;
#pragma unroll
        for (int wi = 0; wi < NW; ++wi) {
            const int j0 = wi * W;
            const unsigned m = j0 < k ? (active >> j0) & kWindowMask : 0u;
            if (m) {
                const float* pw = p + wi * window;
                float* qw = q + wi * window;
                float acc[W];
#pragma unroll
                for (int c = 0; c < W; ++c) acc[c] = 0.0f;
                if (row < n) {
                    row_partial_dot_multi<LANES, W, true>(begin, end, lane, nnz, cols, vals, pw, W, 0, 0, true, acc);
                }
#pragma unroll
                for (int c = 0; c < W; ++c) acc[c] = group_sum<LANES>(acc[c]);
                if (lane == 0 && row < n) {
                    float pv[W];
                    load_own<W>(pw, W, row, 0, pv);
#pragma unroll
                    for (int c = 0; c < W; ++c) pq[wi * W + c] += prod64(pv[c], acc[c]);
                    // (a frozen column inside a running window is computed along: its q and its sum are never read)
                    // (store_own's W / 4 stores written out: through the helper, the NW = 2 instantiations come out
                    // 60 to 72 bytes longer with the same registers)
#pragma unroll
                    for (int g = 0; g < W; g += 4) {
                        const f32x4 v = {acc[g], acc[g + 1], acc[g + 2], acc[g + 3]};
                        *reinterpret_cast<f32x4*>(qw + row * W + g) = v;
                    }
                }
            }
        }
    }
    const double total = block_sum_columns<NW * W>(pq);
    const int j = threadIdx.x;
    if (j < k && ((active >> j) & 1u)) part[part_stride * j + blockIdx.x] = total;
}

// Per column: alpha = rz / p.q; x += alpha p; r -= alpha q; partials of r.z and r.r ->
// part_out[(2 * gridDim.x) * column + 2 * block], z = r * dinv (r where dinv is null).  A thread owns row i of the
// k-wide vectors.  STORED_Z (IC): z does not exist yet and dinv is not read: the partials of r.r alone, into the same
// slot ([... + 1]); r.z follows from cgm_rz_kernel.
template <int W, bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void cgm_update_kernel(int n, int step, int k, const float* __restrict__ p, const float* __restrict__ q,
                       const float* __restrict__ dinv, float* __restrict__ X, long long ldx,
                       float* __restrict__ r, CgMultiState* __restrict__ state, const double* __restrict__ pq_part,
                       int pq_count, long long pq_stride, double* __restrict__ part_out) {
    constexpr int kSums = STORED_Z ? 1 : 2;       // per column: r.r, or r.z and r.r
    const unsigned active = active_columns(state, k);
    if (!active) return;
    const long long out_stride = 2LL * gridDim.x;
    for (int j0 = 0; j0 < k; j0 += W) {
        const unsigned running = (active >> j0) & ((1u << W) - 1u);
        if (!running) continue;
        double pq[W];                 // fold_partials(pq_part + pq_stride * column, pq_count, 1), W columns at once
#pragma unroll
        for (int c = 0; c < W; ++c) pq[c] = 0.0;
        for (int i = threadIdx.x; i < pq_count; i += kBlock) {
#pragma unroll
            for (int c = 0; c < W; ++c) pq[c] += pq_part[pq_stride * (j0 + c) + i];   // (all W: the array is padded)
        }
        fold_values<W>(pq);
        float alpha[W];
        unsigned m = 0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            alpha[c] = 0.0f;
            if (!((running >> c) & 1u)) continue;
            const int j = j0 + c;
            if (!(pq[c] > 0.0)) {          // this column's A is not SPD (or p.q is not finite): its x stays as it is
                if (blockIdx.x == 0 && threadIdx.x == 0) {
                    state->col[j].breakdown = 1;
                    state->col[j].done = 1;
                }
            } else {
                alpha[c] = static_cast<float>(state->col[j].rz[step & 1] / pq[c]);
                m |= 1u << c;
            }
        }
        if (!m) continue;
        double sums[kSums * W];       // r.z, r.r of column j0 + c at [2 * c ..]; STORED_Z: r.r at [c]
#pragma unroll
        for (int c = 0; c < kSums * W; ++c) sums[c] = 0.0;
        const long long window = static_cast<long long>(j0 / W) * n * W;
        const float* pw = p + window;
        const float* qw = q + window;
        float* rw = r + window;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float pv[W], qv[W], rv[W];
            load_own<W>(pw, W, i, 0, pv);
            load_own<W>(qw, W, i, 0, qv);
            load_own<W>(rw, W, i, 0, rv);
            [[maybe_unused]] const float di = dinv ? dinv[i] : 1.0f;      // (STORED_Z: not used, no load)
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if ((m >> c) & 1u) {
                    float* xi = X + i * ldx + j0 + c;
                    *xi = __builtin_fmaf(alpha[c], pv[c], *xi);
                    const float ri = __builtin_fmaf(-alpha[c], qv[c], rv[c]);
                    rw[i * W + c] = ri;
                    if constexpr (STORED_Z) {
                        sums[c] += prod64(ri, ri);
                    } else {
                        const float zi = dinv ? __fmul_rn(ri, di) : ri;
                        sums[2 * c] += prod64(ri, zi);
                        sums[2 * c + 1] += prod64(ri, ri);
                    }
                }
            }
        }
        const double total = block_sum_columns<kSums * W>(sums);
        const int c = threadIdx.x / kSums;
        if (c < W && ((m >> c) & 1u)) {
            part_out[out_stride * (j0 + c) + 2LL * blockIdx.x + (STORED_Z ? 1 : threadIdx.x % 2)] = total;
        }
    }
}

// Per column: beta = rz_new / rz_old, the stop test, p = z + beta p.  Workgroup 0 commits each column's step and,
// once no column is left, the global flag.  zr is R and z = r * dinv (r where dinv is null), or with STORED_Z it is Z
// itself and dinv is not read.
template <int W, bool STORED_Z>
__global__ __launch_bounds__(kBlock)
void cgm_direction_kernel(int n, int step, int k, const float* __restrict__ zr, const float* __restrict__ dinv,
                          float* __restrict__ p, CgMultiState* __restrict__ state,
                          const double* __restrict__ part, int count) {
    const unsigned active = active_columns(state, k);
    if (!active) return;
    const bool commits = blockIdx.x == 0 && threadIdx.x == 0;
    int finished = k - __popc(active);
    for (int j0 = 0; j0 < k; j0 += W) {
        const unsigned running = (active >> j0) & ((1u << W) - 1u);
        if (!running) continue;
        double sums[2 * W];           // fold_partials(part + 2 * count * column, count, 2): r.z, r.r at [2 * c ..]
#pragma unroll
        for (int c = 0; c < 2 * W; ++c) sums[c] = 0.0;
        for (int i = threadIdx.x; i < count; i += kBlock) {
#pragma unroll
            for (int c = 0; c < W; ++c) {         // (all W: the array is padded)
                const double* mine = part + 2LL * count * (j0 + c) + 2LL * i;
                sums[2 * c] += mine[0];
                sums[2 * c + 1] += mine[1];
            }
        }
        fold_values<2 * W>(sums);
        float beta[W];
        unsigned m = 0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            beta[c] = 0.0f;
            if (!((running >> c) & 1u)) continue;
            CgColumn& col = state->col[j0 + c];
            const double rz = sums[2 * c], rr = sums[2 * c + 1];
            const double res = sqrt(rr);
            const bool converged = res <= col.threshold;
            const bool breakdown = !converged && !(rz > 0.0);
            const double rz_old = col.rz[step & 1];
            if (commits) {
                col.iterations = step + 1;
                col.relative_residual = static_cast<float>(res / col.bnorm);
                col.rz[(step + 1) & 1] = rz;
                if (converged) col.converged = 1;
                if (breakdown) col.breakdown = 1;
                if (converged || breakdown) col.done = 1;
            }
            if (converged || breakdown) {
                ++finished;
            } else {
                beta[c] = static_cast<float>(rz / rz_old);
                m |= 1u << c;
            }
        }
        if (!m) continue;
        const long long window = static_cast<long long>(j0 / W) * n * W;
        const float* zw = zr + window;
        float* pw = p + window;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float zv[W], pv[W];
            load_own<W>(zw, W, i, 0, zv);
            load_own<W>(pw, W, i, 0, pv);
            [[maybe_unused]] const float di = dinv ? dinv[i] : 1.0f;      // (STORED_Z: not used, no load)
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if ((m >> c) & 1u) {
                    float zi = zv[c];
                    if constexpr (!STORED_Z) zi = dinv ? __fmul_rn(zi, di) : zi;
                    pw[i * W + c] = __builtin_fmaf(beta[c], pv[c], zi);
                }
            }
        }
    }
    if (commits && finished == k) state->done = 1;
}

// IC: per column the block partials of r.z -> part[col_stride * column + stride * block] (stride 2 and the loop's
// grid inside the loop, stride 3 and the row grid over the init partials, as cg.hip's cg_rz_kernel).
template <int W>
__global__ __launch_bounds__(kBlock)
void cgm_rz_kernel(int n, int k, const float* __restrict__ r, const float* __restrict__ z,
                   const CgMultiState* __restrict__ state, double* __restrict__ part, long long col_stride,
                   int stride) {
    const unsigned active = active_columns(state, k);
    if (!active) return;
    for (int j0 = 0; j0 < k; j0 += W) {
        const unsigned running = (active >> j0) & ((1u << W) - 1u);
        if (!running) continue;
        double sums[W];
#pragma unroll
        for (int c = 0; c < W; ++c) sums[c] = 0.0;
        const long long window = static_cast<long long>(j0 / W) * n * W;
        const float* rw = r + window;
        const float* zw = z + window;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float rv[W], zv[W];
            load_own<W>(rw, W, i, 0, rv);
            load_own<W>(zw, W, i, 0, zv);
#pragma unroll
            for (int c = 0; c < W; ++c) sums[c] += prod64(rv[c], zv[c]);
        }
        const double total = block_sum_columns<W>(sums);
        const int c = threadIdx.x;
        if (c < W && ((running >> c) & 1u)) {
            part[col_stride * (j0 + c) + static_cast<long long>(stride) * blockIdx.x] = total;
        }
    }
}

struct Shape {
    const CSRMatrix* A;
    int k;
    int w;                    // columns per window of the workspace: 4 up to k = 4, else 8
};

// windows of 4 columns of B and X at every k: with 8, the guards of the caller's B and X push scalar registers out
hipError_t init(int lanes, const Shape& sh, const float* B, int ldb, const float* X, int ldx, const float* dinv,
                float* r, float* p, double* part, int grid, hipStream_t s) {
    const CSRMatrix* A = sh.A;
    const bool x_vec = ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    return with_lanes(lanes, [&](auto L) {
        return with_window(sh.w, [&](auto WS) {
            cgm_init_kernel<decltype(L)::value, 4, decltype(WS)::value><<<grid, kBlock, 0, s>>>(
                A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, B, ldb, X, ldx, x_vec, sh.k, dinv, r,
                p, part);
            return hipGetLastError();
        });
    });
}

template <int LANES, int W, int NW>
hipError_t launch_spmv_dot(const Shape& sh, const float* p, float* q, const CgMultiState* state, double* part,
                           int grid, hipStream_t s) {
    const CSRMatrix* A = sh.A;
    cgm_spmv_dot<LANES, W, NW><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices,
                                                       A->d_values, p, q, sh.k, state, part, grid);
    return hipGetLastError();
}

// windows: one of 4 columns up to k = 4, then 1, 2 or 4 of 8 columns
hipError_t spmv_dot(int lanes, const Shape& sh, const float* p, float* q, const CgMultiState* state, double* part,
                    int grid, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        constexpr int kLanes = decltype(L)::value;
        if (sh.k <= 4) return launch_spmv_dot<kLanes, 4, 1>(sh, p, q, state, part, grid, s);
        if (sh.k <= 8) return launch_spmv_dot<kLanes, 8, 1>(sh, p, q, state, part, grid, s);
        if (sh.k <= 16) return launch_spmv_dot<kLanes, 8, 2>(sh, p, q, state, part, grid, s);
        return launch_spmv_dot<kLanes, 8, 4>(sh, p, q, state, part, grid, s);
    });
}

// the floats [a, a + na) and [b, b + nb) share a byte
bool spans_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) &&
           b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

// F: the factor matrix of cg_solve_multi_ic (with_ic), not read otherwise
int solve_multi(const CSRMatrix* A, bool with_ic, const CSRMatrix* F, const float* d_B, int ldb, float* d_X, int ldx,
                int k, const CGConfig* config, CGResult* results) {
    const auto fail = [&](SpMVError e) {
        if (results && k >= 1 && k <= kMaxColumns) {       // a k out of range says nothing about the array's length
            for (int j = 0; j < k; ++j) results[j].error_code = code(e);
        }
        return code(e);
    };
    if (!A || !d_B || !d_X || !results) return fail(SpMVError::INVALID_ARGUMENT);
    if (k < 1 || k > kMaxColumns) return fail(SpMVError::INVALID_ARGUMENT);
    if (ldb < k || ldx < k) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return fail(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        for (int j = 0; j < k; ++j) {
            results[j] = CGResult();
            results[j].converged = 1;
        }
        return code(SpMVError::SUCCESS);
    }
    if (!device_arrays(A)) return fail(SpMVError::INVALID_FORMAT);
    const CGConfig defaults;
    const CGConfig& cfg = config ? *config : defaults;
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 ||
        (!with_ic && cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI) ||
        cfg.engine < -1 || cfg.engine > 0) {          // the LDS-tiled engine has no k-wide form
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const int n = A->num_rows;
    if (spans_overlap(d_B, static_cast<long long>(n - 1) * ldb + k, d_X, static_cast<long long>(n - 1) * ldx + k)) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    if (with_ic) {
        if (!F) return fail(SpMVError::INVALID_ARGUMENT);
        if (F->num_rows != F->num_cols || F->num_rows != n) return fail(SpMVError::INVALID_DIMENSION);
        if (!device_arrays(F)) return fail(SpMVError::INVALID_FORMAT);
    }

    const TraceRange range(with_ic ? "spmv:cg_solve_multi_ic" : "spmv:cg_solve_multi");
    hipStream_t stream = current_stream();
    const bool jacobi = !with_ic && cfg.preconditioner == CGConfig::JACOBI;

    TriangularPair ic;                // M = L L^T: the lower solve reads L's stored diagonal
    if (with_ic) {
        const int status = ic.build(F, 0, stream);
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const size_t pq_count = static_cast<size_t>(row_grid);
    const size_t rr_count = 2 * static_cast<size_t>(vgrid);
    const size_t init_count = 3 * static_cast<size_t>(row_grid);
    const Shape sh{A, k, k <= 4 ? 4 : 8};

    Workspace<CgMultiState> ws;       // R, P, Q (ceil(k / w) windows of n x w each) and dinv (JACOBI) or Z (IC)
    const size_t len = static_cast<size_t>(n) * static_cast<size_t>((k + sh.w - 1) / sh.w * sh.w);
    const size_t k_pad = len / static_cast<size_t>(n);       // whole windows: the folds read all W columns of one
    if (!ws.allocate(3 * len + (jacobi ? static_cast<size_t>(n) : with_ic ? len : 0),
                     k_pad * (pq_count + rr_count) + static_cast<size_t>(k) * init_count)) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    float* r = ws.vec;
    float* p = ws.vec + len;
    float* q = ws.vec + 2 * len;
    float* dinv = jacobi ? ws.vec + 3 * len : nullptr;
    float* z = with_ic ? ws.vec + 3 * len : nullptr;
    double* pq_part = ws.part;
    double* rr_part = pq_part + k_pad * pq_count;
    double* init_part = rr_part + k_pad * rr_count;
    CgMultiState* pinned = ws.pinned;
    // Z = L^-T (L^-1 R) on the windowed workspace, whole windows (the padding columns are solved along and never used)
    const auto apply_ic = [&]() -> bool {
        const long long window = static_cast<long long>(n) * sh.w;
        const SptrsvMultiArrays down{r, sh.w, window, z, sh.w, window, static_cast<int>(k_pad), sh.w};
        const SptrsvMultiArrays up{z, sh.w, window, z, sh.w, window, static_cast<int>(k_pad), sh.w};
        return ic.apply(down, up, stream);
    };

    // setup: the shared diagonal, R0 / P0 and their dots, the column states; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(CgMultiState), stream) == hipSuccess;
    int* bad = &ws.state->bad_diagonal;
    if (jacobi) ok = ok && launch_diag<DiagRule::POSITIVE>(A, dinv, bad, stream) == hipSuccess;
    if (with_ic) ok = ok && launch_diag<DiagRule::POSITIVE_FINITE>(F, nullptr, bad, stream) == hipSuccess;
    ok = ok && init(lanes, sh, d_B, ldb, d_X, ldx, dinv, r, p, init_part, row_grid, stream) == hipSuccess;
    if (ok && with_ic) {
        // the init kernel left P0 = R0 and r0.r0 in the r.z slots: Z0 = M^-1 R0, the true r0.z0 over them, P0 = Z0
        ok = apply_ic();
        if (ok) {
            ok = with_window(sh.w, [&](auto W) {
                cgm_rz_kernel<decltype(W)::value><<<row_grid, kBlock, 0, stream>>>(n, k, r, z, ws.state, init_part,
                                                                                   3LL * row_grid, 3);
                return hipGetLastError();
            }) == hipSuccess &&
                 hipMemcpyAsync(p, z, len * sizeof(float), hipMemcpyDeviceToDevice, stream) == hipSuccess;
        }
    }
    if (ok) {
        cgm_start_kernel<<<1, kBlock, 0, stream>>>(init_part, row_grid, k, cfg.tolerance, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (pinned[0].bad_diagonal) return fail(SpMVError::INVALID_ARGUMENT);
    bool any_zero_b = false;
    for (int j = 0; j < k; ++j) any_zero_b = any_zero_b || pinned[0].col[j].zero_b;
    if (any_zero_b) {
        cgm_zero_kernel<<<vec_grid(static_cast<long long>(n) * k), kBlock, 0, stream>>>(n, k, d_X, ldx, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }

    float elapsed_ms = 0.0f;
    const bool run_loop = !pinned[0].done;
    if (ok && run_loop) {
        EventPair& ev = thread_events();
        ok = hipEventRecord(ev.start, stream) == hipSuccess;
        for (int iter = 0; ok && iter < cfg.max_iterations; ++iter) {
            const TraceRange step_range("spmv:cg_multi_step");
            ok = spmv_dot(lanes, sh, p, q, ws.state, pq_part, row_grid, stream) == hipSuccess;
            if (ok && with_ic) {
                ok = with_window(sh.w, [&](auto W) {
                    cgm_update_kernel<decltype(W)::value, true><<<vgrid, kBlock, 0, stream>>>(
                        n, iter, k, p, q, nullptr, d_X, ldx, r, ws.state, pq_part, row_grid, row_grid, rr_part);
                    return hipGetLastError();
                }) == hipSuccess && apply_ic();
            }
            if (ok) {
                // the host needs the global flag alone per step: the header in front of the column states
                ok = with_window(sh.w, [&](auto WC) {
                    constexpr int W = decltype(WC)::value;
                    if (with_ic) {
                        cgm_rz_kernel<W><<<vgrid, kBlock, 0, stream>>>(n, k, r, z, ws.state, rr_part, 2LL * vgrid, 2);
                        cgm_direction_kernel<W, true><<<vgrid, kBlock, 0, stream>>>(n, iter, k, z, nullptr, p, ws.state,
                                                                                    rr_part, vgrid);
                    } else {
                        cgm_update_kernel<W, false><<<vgrid, kBlock, 0, stream>>>(
                            n, iter, k, p, q, dinv, d_X, ldx, r, ws.state, pq_part, row_grid, row_grid, rr_part);
                        cgm_direction_kernel<W, false><<<vgrid, kBlock, 0, stream>>>(n, iter, k, r, dinv, p, ws.state,
                                                                                     rr_part, vgrid);
                    }
                    return hipGetLastError();
                }) == hipSuccess && ws.publish(iter, kHeaderBytes, stream);
            }
            if (ok && iter >= 1) {
                const CgMultiState* seen = ws.wait_previous(iter);
                ok = seen != nullptr;
                if (ok && seen->done) break;
            }
        }
        ok = ws.finish_timed(ok, ev, stream, &elapsed_ms);
    } else if (ok) {
        ok = hipStreamSynchronize(stream) == hipSuccess;      // the zero columns, if any
    }
    if (!ok) {
        (void)hipGetLastError();
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    for (int j = 0; j < k; ++j) {
        const CgColumn& c = pinned[0].col[j];
        CGResult out;
        out.iterations = c.iterations;
        out.relative_residual = c.relative_residual;
        out.converged = c.converged;
        out.breakdown = c.breakdown;
        out.elapsed_ms = elapsed_ms;
        results[j] = out;
    }
    return code(SpMVError::SUCCESS);
}

} // namespace
} // namespace detail

int cg_solve_multi(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                   const CGConfig* config, CGResult* results) {
    return detail::solve_multi(A, false, nullptr, d_B, ldb, d_X, ldx, k, config, results);
}

int cg_solve_multi_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_B, int ldb, float* d_X, int ldx, int k,
                      const CGConfig* config, CGResult* results) {
    return detail::solve_multi(A, true, F, d_B, ldb, d_X, ldx, k, config, results);
}

} // namespace spmv
