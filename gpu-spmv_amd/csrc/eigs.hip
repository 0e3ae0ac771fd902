// eigs.hip — device-resident thick-restart Lanczos (include/spmv/eigs.h).
//
// Built like gmres.hip: the projected matrix T, the Ritz decomposition and the stop tests live in device memory, every
// gated kernel returns at once when the state says so, and inside a cycle the host reads a two-deep pinned mirror of
// the state so that it enqueues step j+1 before it looks at the outcome of step j.  The state has two phases: `open`
// (the cycle accepts Lanczos steps) and closed (it waits for its close sequence); step kernels run only while open,
// close kernels only while closed and only for the decision they belong to.  A cycle close is where the host waits:
// it reads the decision of eigs_ritz (and of eigs_verdict) back and enqueues the one sequence that applies.
//
// A step, column j (the basis vectors v_0..v_j are ready):
//   eigs_spmv<LANES> / tiled_spmv     w = A v_j
//   eigs_multidot                     one pass over w and v_0..v_j: (j+1) partials per workgroup of h1_i = v_i.w
//   eigs_update_multidot              folds h1, w -= h1_i v_i, then the partials of h2_i = v_i.w on the updated w
//   eigs_update_norm                  folds h2, w -= h2_i v_i, and the partials of w.w
//   eigs_column (one workgroup)       folds w.w; commits column j of T, beta, the invariance and close tests, 1 / beta
//   eigs_normalize                    v_j+1 = w * scale
// The close of a cycle with c columns:
//   eigs_ritz (one workgroup)         T -> LDS, cyclic Jacobi (sym_eig_small's device form), the sort by `which`, the
//                                     estimates, the fp32 coefficients, and the decision FINISH / RESTART with p
//   FINISH:  eigs_rotate<true>        y_i = sum_l S[l,i] v_l into the caller's d_vectors, zeros for the pairs not found
//            per returned pair: eigs_spmv<LANES> (finish mode) t = A y_i, eigs_residual_partials
//            eigs_verdict (one workgroup): r_i, d_values, d_residuals, converged; done, or RESTART after all
//   RESTART: eigs_rotate<false>       v_i <- sum_l S[l,i] v_l for i < p in place, v_p <- v_c
//            eigs_restart (one workgroup): T <- diag(theta), c <- p, the cycle is open again
// A one-workgroup kernel is the only writer of the state, and no kernel reads a state field that a kernel of the same
// launch writes.  T (at most 32 KB) lives in LDS during the Jacobi sweeps, padded to a stride of 65 doubles so that
// both the column and the row phase of a round are free of bank conflicts; S lives in global memory, stored by
// columns: a round touches every column once, with contiguous accesses, nobody reads a value another thread of the
// same phase writes, and the rotation kernels read S from global memory anyway.
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"
#include "basis_ops.h"
#include "eigs_impl.h"
#include "generators.h"
#include "tiled.h"
#include "spmv/eigs.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;
using namespace basis;
using namespace eigs;

constexpr int kMaxBasis = kMaxOrder;
constexpr int kLdsStride = kMaxOrder + 1;      // T in LDS: both phases of a round conflict-free
enum Decision { UNDECIDED = 0, FINISH = 1, RESTART = 2 };

// Lives in device memory and is mirrored to the host.
struct EigsState {
    double beta;              // sqrt(w.w) of the last committed column
    double theta_max;         // max |theta| over the Ritz values of the last close
    double max_residual;      // of the last finish
    float  scale;             // 1 / beta_0 (eigs_start) or 1 / beta (eigs_column): what eigs_normalize applies
    int    iterations;        // committed columns over all cycles
    int    restarts;
    int    jc;                // columns of T in this cycle
    int    next;              // the basis vector eigs_normalize is to write
    int    open;              // 1: the cycle accepts steps; 0: it waits for its close sequence
    int    decision;          // Decision of the close in flight
    int    p;                 // vectors a thick restart keeps
    int    found;             // pairs a finish returns: min(k, jc)
    int    invariant;         // the space is invariant (or the whole one)
    int    converged;
    int    breakdown;         // EigsResult::Breakdown
    int    done;              // everything after this is a no-op
    int    bad_start;         // the start vector is zero
};

// work arrays of the small problem, in one allocation
struct Small {
    double* T;        // kMaxBasis x kMaxBasis, T[i * kMaxBasis + j], both triangles
    double* S;        // by columns: S[col * kMaxBasis + l]
    double* theta;    // sorted by `which`
    float*  C;        // C[i * kMaxBasis + l] = fp32(S[l, order[i]])
    float*  theta32;
    float*  h1;
    float*  h2;
};
constexpr size_t kSmallDoubles = 2 * kMaxBasis * kMaxBasis + kMaxBasis +
                                 ((kMaxBasis * kMaxBasis + 3 * kMaxBasis) * sizeof(float)) / sizeof(double);

__device__ __forceinline__ bool stepping(const EigsState* st) { return st->open && !st->done; }
__device__ __forceinline__ bool closing(const EigsState* st, int decision) {
    return !st->open && !st->done && st->decision == decision;
}

// ---- the small eigen-solve: one workgroup ------------------------------------------------------------------------

// W: n x n in LDS (stride kLdsStride), S: n columns of n in global memory (stride kMaxBasis), S = I on entry.
// include/spmv/eigs.h's rule; eigs_host.cpp's sym_eig_small_host is the same operations one after another.
__device__ __forceinline__ void jacobi_sweeps(int n, double* W, double* __restrict__ S) {
    __shared__ double s_c[kMaxOrder / 2], s_s[kMaxOrder / 2];
    __shared__ int s_p[kMaxOrder / 2], s_q[kMaxOrder / 2];
    __shared__ double s_max[kBlock / 64];
    __shared__ int s_any;
    const int tid = threadIdx.x;
    double mx = 0.0;
    for (int idx = tid; idx < n * n; idx += kBlock) mx = fmax(mx, fabs(W[(idx / n) * kLdsStride + idx % n]));
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) s_max[tid >> 6] = mx;
    __syncthreads();
    double scale = s_max[0];
    for (int w = 1; w < kBlock / 64; ++w) scale = fmax(scale, s_max[w]);
    const double thr = scale * 0x1p-53;
    const int N = (n + 1) & ~1;
    const int half = N / 2;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        __syncthreads();
        if (tid == 0) s_any = 0;
        __syncthreads();
        for (int r = 0; r < N - 1; ++r) {
            if (tid < half) {
                int p, q;
                round_robin_pair(r, tid, N, p, q);
                int active = -1;
                if (q < n) {
                    const double apq = W[p * kLdsStride + q];
                    if (fabs(apq) > thr) {
                        double c, s;
                        rotation(W[p * kLdsStride + p], W[q * kLdsStride + q], apq, c, s);
                        s_c[tid] = c;
                        s_s[tid] = s;
                        s_q[tid] = q;
                        active = p;
                        s_any = 1;
                    }
                }
                s_p[tid] = active;
            }
            __syncthreads();
            for (int t = tid; t < half * n; t += kBlock) {         // columns of W and of S
                const int k = t / n, i = t % n;
                const int p = s_p[k];
                if (p < 0) continue;
                const int q = s_q[k];
                const double c = s_c[k], s = s_s[k];
                double x = W[i * kLdsStride + p], y = W[i * kLdsStride + q];
                rotate_pair(c, s, x, y);
                W[i * kLdsStride + p] = x;
                W[i * kLdsStride + q] = y;
                x = S[p * kMaxBasis + i];
                y = S[q * kMaxBasis + i];
                rotate_pair(c, s, x, y);
                S[p * kMaxBasis + i] = x;
                S[q * kMaxBasis + i] = y;
            }
            __syncthreads();
            for (int t = tid; t < half * n; t += kBlock) {         // rows of W
                const int k = t / n, j = t % n;
                const int p = s_p[k];
                if (p < 0) continue;
                const int q = s_q[k];
                double x = W[p * kLdsStride + j], y = W[q * kLdsStride + j];
                rotate_pair(s_c[k], s_s[k], x, y);
                W[p * kLdsStride + j] = x;
                W[q * kLdsStride + j] = y;
            }
            __syncthreads();
            if (tid < half && s_p[tid] >= 0) {
                W[s_p[tid] * kLdsStride + s_q[tid]] = 0.0;
                W[s_q[tid] * kLdsStride + s_p[tid]] = 0.0;
            }
            __syncthreads();
        }
        if (!s_any) break;          // uniform: read after the round's last barrier, reset after the next one
    }
    __syncthreads();
}

// W <- T[0:n, 0:n], S <- I
__device__ __forceinline__ void load_small(int n, const double* __restrict__ T, double* W, double* __restrict__ S) {
    for (int idx = threadIdx.x; idx < n * n; idx += kBlock) {
        const int i = idx / n, j = idx % n;
        W[i * kLdsStride + j] = T[i * kMaxBasis + j];
        S[i * kMaxBasis + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
}

// s_order[rank] = the diagonal position of the rank-th value: ascending (descending != 0: descending), ties by position
__device__ __forceinline__ void rank_diagonal(int n, const double* W, int descending, int* s_order) {
    if (threadIdx.x < n) {
        const int i = threadIdx.x;
        const double di = W[i * kLdsStride + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double dj = W[j * kLdsStride + j];
            rank += ((descending ? dj > di : dj < di) || (dj == di && j < i)) ? 1 : 0;
        }
        s_order[rank] = i;
    }
    __syncthreads();
}

// sym_eig_small with on_device: T and vectors at stride kMaxBasis
__global__ __launch_bounds__(kBlock)
void sym_eig_small_kernel(int n, const double* __restrict__ T, double* __restrict__ S, double* __restrict__ values,
                          double* __restrict__ vectors) {
    __shared__ double W[kMaxOrder * kLdsStride];
    __shared__ int s_order[kMaxOrder];
    load_small(n, T, W, S);
    jacobi_sweeps(n, W, S);
    rank_diagonal(n, W, 0, s_order);
    if (threadIdx.x < n) values[threadIdx.x] = W[s_order[threadIdx.x] * kLdsStride + s_order[threadIdx.x]];
    for (int idx = threadIdx.x; idx < n * n; idx += kBlock) {
        const int i = idx / n, l = idx % n;
        vectors[i * kMaxBasis + l] = S[s_order[i] * kMaxBasis + l];
    }
}

// ---- the step ----------------------------------------------------------------------------------------------------

// w = A v (vector CSR).  FINISHING: t = A y_i of the finish, for pair `pair` < found; else while a cycle is open.
template <int LANES, bool FINISHING>
__global__ __launch_bounds__(kBlock)
void eigs_spmv(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
               const float* __restrict__ vals, const float* __restrict__ v, float* __restrict__ w, int pair,
               const EigsState* __restrict__ st) {
    if (FINISHING ? !(closing(st, FINISH) && pair < st->found) : !stepping(st)) return;
    for_each_row_dot<LANES>(n, nnz, row_ptrs, cols, vals, v, [&](long long row, float sum) { w[row] = sum; });
}

__global__ __launch_bounds__(kBlock)
void eigs_multidot(long long n, long long ld, int j, const float* __restrict__ V, const float* __restrict__ w,
                   const EigsState* __restrict__ st, double* __restrict__ part1) {
    if (!stepping(st)) return;
    multidot_pass(n, ld, j + 1, V, w, part1);
}

__global__ __launch_bounds__(kBlock)
void eigs_update_multidot(long long n, long long ld, int j, const float* __restrict__ V, float* w,
                          const EigsState* __restrict__ st, const double* __restrict__ part1,
                          float* __restrict__ h1, double* __restrict__ part2) {
    if (!stepping(st)) return;
    __shared__ float s_h[kMaxBasis];
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
void eigs_update_norm(long long n, long long ld, int j, const float* __restrict__ V, float* w,
                      const EigsState* __restrict__ st, const double* __restrict__ part2,
                      float* __restrict__ h2, double* __restrict__ ww_part) {
    if (!stepping(st)) return;
    __shared__ float s_h[kMaxBasis];
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

// One workgroup.  Column j: h_i = double(fp32 h1_i) + double(fp32 h2_i), beta = sqrt(w.w); commits the column to both
// triangles of T; the invariance test; closes the cycle, or leaves 1 / beta for eigs_normalize.
__global__ __launch_bounds__(kBlock)
void eigs_column(int j, int m, int n, int max_iterations, const double* __restrict__ ww_part, int ww_count, Small sm,
                 EigsState* __restrict__ st) {
    if (!stepping(st)) return;
    __shared__ double s_col[kMaxBasis];
    double ww = 0.0, unused = 0.0;
    fold_partials(ww_part, ww_count, 1, ww, unused);
    if (threadIdx.x <= j) {
        s_col[threadIdx.x] = static_cast<double>(sm.h1[threadIdx.x]) + static_cast<double>(sm.h2[threadIdx.x]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double beta = sqrt(ww);
    bool finite = isfinite(beta);
    double hmax = 0.0;
    for (int i = 0; i <= j; ++i) {
        finite = finite && isfinite(s_col[i]);
        hmax = fmax(hmax, fabs(s_col[i]));
    }
    if (!finite) {
        st->breakdown = EigsResult::NOT_FINITE;
        st->open = 0;
        st->done = 1;
        return;
    }
    for (int i = 0; i <= j; ++i) {
        sm.T[i * kMaxBasis + j] = s_col[i];
        sm.T[j * kMaxBasis + i] = s_col[i];
    }
    const int total = st->iterations + 1;
    st->iterations = total;
    st->jc = j + 1;
    st->beta = beta;
    const bool invariant = beta <= hmax * 0x1p-20 || j + 1 == n;
    if (invariant) {
        st->invariant = 1;
    } else {
        st->scale = static_cast<float>(1.0 / beta);
        st->next = j + 1;
    }
    if (invariant || j + 1 == m || total >= max_iterations) st->open = 0;
}

// v_next = src * scale, when eigs_start (next == 0) or eigs_column (next == j + 1) has just asked for it.  src may be
// the caller's start vector: scalar accesses.
__global__ __launch_bounds__(kBlock)
void eigs_normalize(long long n, int next, const float* __restrict__ src, float* __restrict__ dst,
                    const EigsState* __restrict__ st) {
    if (st->done || st->next != next || st->jc != next) return;
    const float scale = st->scale;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        dst[i] = __fmul_rn(src[i], scale);
    }
}

// ---- setup -------------------------------------------------------------------------------------------------------

// part[2 * block] = this workgroup's share of x.x (x may be misaligned)
__global__ __launch_bounds__(kBlock)
void eigs_norm_partials(long long n, const float* __restrict__ x, double* __restrict__ part) {
    double xx = 0.0, unused = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        xx += prod64(x[i], x[i]);
    }
    block_sum2(xx, unused);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = xx;
        part[2 * blockIdx.x + 1] = 0.0;
    }
}

// One workgroup: beta_0 of the start vector; opens the first cycle (with max_iterations == 0 the cycle stays closed and
// its close finishes with no pair).  The state was zeroed before.
__global__ __launch_bounds__(kBlock)
void eigs_start(const double* __restrict__ part, int count, int max_iterations, EigsState* __restrict__ st) {
    double xx = 0.0, unused = 0.0;
    fold_partials(part, count, 2, xx, unused);
    if (threadIdx.x != 0) return;
    const double beta = sqrt(xx);
    if (!isfinite(beta)) {
        st->breakdown = EigsResult::NOT_FINITE;
        st->done = 1;
    } else if (beta == 0.0) {
        st->bad_start = 1;
        st->done = 1;
    } else {
        st->scale = static_cast<float>(1.0 / beta);
        st->open = max_iterations > 0 ? 1 : 0;
    }
}

// ---- the close ---------------------------------------------------------------------------------------------------

// One workgroup.  The Ritz decomposition of T[0:c, 0:c], the sort by `which`, the estimates |beta S[c-1, i]|, the fp32
// coefficients of the rotations, and the decision.
__global__ __launch_bounds__(kBlock)
void eigs_ritz(int k, int which, int m, int max_iterations, float tolerance, Small sm, EigsState* __restrict__ st) {
    if (!closing(st, UNDECIDED)) return;
    __shared__ double W[kMaxOrder * kLdsStride];
    __shared__ int s_order[kMaxOrder];
    __shared__ double s_est[kMaxOrder];
    const int c = st->jc;
    if (c == 0) {                                   // max_iterations == 0: nothing to decompose
        if (threadIdx.x == 0) {
            st->found = 0;
            st->theta_max = 0.0;
            st->decision = FINISH;
        }
        return;
    }
    load_small(c, sm.T, W, sm.S);
    jacobi_sweeps(c, W, sm.S);
    rank_diagonal(c, W, which == EigsConfig::LARGEST, s_order);
    const double beta = st->beta;
    if (threadIdx.x < c) {
        const int col = s_order[threadIdx.x];
        const double theta = W[col * kLdsStride + col];
        sm.theta[threadIdx.x] = theta;
        sm.theta32[threadIdx.x] = static_cast<float>(theta);
        s_est[threadIdx.x] = fabs(__dmul_rn(beta, sm.S[col * kMaxBasis + (c - 1)]));
    }
    for (int idx = threadIdx.x; idx < c * c; idx += kBlock) {
        const int i = idx / c, l = idx % c;
        sm.C[i * kMaxBasis + l] = static_cast<float>(sm.S[s_order[i] * kMaxBasis + l]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double theta_max = 0.0;
    for (int i = 0; i < c; ++i) theta_max = fmax(theta_max, fabs(W[i * kLdsStride + i]));
    const double threshold = __dmul_rn(static_cast<double>(tolerance), theta_max);
    bool pass = c >= k;
    for (int i = 0; i < k && i < c; ++i) pass = pass && s_est[i] <= threshold;
    st->theta_max = theta_max;
    st->found = min(k, c);
    st->p = min(k + (m - k) / 2, c - 1);
    st->decision = pass || st->iterations >= max_iterations || st->invariant ? FINISH : RESTART;
}

// out_i = fp32(sum over l < c ascending of double(C[i][l]) * double(v_l)), one thread per element: the thread holds
// its element of all c <= 64 basis vectors in registers (compile-time indexing, predicated on l < c), the fp32
// coefficients sit in LDS.  OUT: the `found` wanted vectors into the caller's array (any alignment: scalar stores),
// zeros for the pairs not found.  Else the thick restart in place — the thread has read everything its outputs depend
// on before it writes — and v_p <- v_c.
template <bool OUT>
__global__ __launch_bounds__(kBlock)
void eigs_rotate(long long n, long long ld, float* V, const float* __restrict__ C, const EigsState* __restrict__ st,
                 float* out, long long ldo, int k) {
    if (!closing(st, OUT ? FINISH : RESTART)) return;
    __shared__ float s_coef[kMaxBasis * kMaxBasis];
    const int c = st->jc;
    const int count = OUT ? st->found : st->p;
    for (int idx = threadIdx.x; idx < count * kMaxBasis; idx += kBlock) {
        s_coef[idx] = idx % kMaxBasis < c ? C[idx] : 0.0f;
    }
    __syncthreads();
    for (long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; e < n;
         e += static_cast<long long>(gridDim.x) * kBlock) {
        float x[kMaxBasis];
#pragma unroll
        for (int l = 0; l < kMaxBasis; ++l) x[l] = l < c ? V[l * ld + e] : 0.0f;
        const float next = OUT ? 0.0f : V[c * ld + e];
        for (int i = 0; i < count; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < kMaxBasis; ++l) {
                if (l < c) acc += prod64(s_coef[i * kMaxBasis + l], x[l]);
            }
            if (OUT) out[i * ldo + e] = static_cast<float>(acc);
            else V[i * ld + e] = static_cast<float>(acc);
        }
        if (OUT) {
            for (int i = count; i < k; ++i) out[i * ldo + e] = 0.0f;
        } else {
            V[count * ld + e] = next;
        }
    }
}

// part[2 * block], part[2 * block + 1] = this workgroup's shares of d.d and y.y, d_e = fmaf(-theta, y_e, t_e)
__global__ __launch_bounds__(kBlock)
void eigs_residual_partials(long long n, const float* __restrict__ t, const float* __restrict__ y, int pair,
                            const float* __restrict__ theta32, const EigsState* __restrict__ st,
                            double* __restrict__ part) {
    if (!(closing(st, FINISH) && pair < st->found)) return;
    const float theta = theta32[pair];
    double dd = 0.0, yy = 0.0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const float yi = y[i];
        const float d = __builtin_fmaf(-theta, yi, t[i]);
        dd += prod64(d, d);
        yy += prod64(yi, yi);
    }
    block_sum2(dd, yy);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = dd;
        part[2 * blockIdx.x + 1] = yy;
    }
}

// One workgroup: the recomputed residuals, the outputs, `converged`; ends the call, or asks for the restart after all.
__global__ __launch_bounds__(kBlock)
void eigs_verdict(int k, float tolerance, int max_iterations, const double* __restrict__ part, int count, Small sm,
                  float* __restrict__ d_values, float* __restrict__ d_residuals, EigsState* __restrict__ st) {
    if (!closing(st, FINISH)) return;
    __shared__ double s_r[kMaxValues];
    const int found = st->found;
    for (int i = 0; i < found; ++i) {
        double dd = 0.0, yy = 0.0;
        fold_partials(part + 2LL * i * count, count, 2, dd, yy);
        if (threadIdx.x == 0) s_r[i] = sqrt(dd);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double threshold = __dmul_rn(static_cast<double>(tolerance), st->theta_max);
    int converged = 0;
    double worst = 0.0;
    const float nan = __builtin_nanf("");
    for (int i = 0; i < k; ++i) {
        if (i < found) {
            converged += s_r[i] <= threshold ? 1 : 0;
            worst = s_r[i] > worst || s_r[i] != s_r[i] ? s_r[i] : worst;
        }
        d_values[i] = i < found ? sm.theta32[i] : nan;
        if (d_residuals) d_residuals[i] = i < found ? static_cast<float>(s_r[i]) : nan;
    }
    st->converged = converged;
    st->max_residual = worst;
    if (converged == k || st->iterations >= max_iterations || st->invariant) {
        if (st->invariant && found < k) st->breakdown = EigsResult::INVARIANT_SUBSPACE;
        st->done = 1;
    } else {
        st->decision = RESTART;
    }
}

// One workgroup: T <- diag(theta_0..theta_p-1), the cycle goes on at column p.
__global__ __launch_bounds__(kBlock)
void eigs_restart(Small sm, EigsState* __restrict__ st) {
    if (!closing(st, RESTART)) return;
    const int p = st->p;
    for (int idx = threadIdx.x; idx < kMaxBasis * kMaxBasis; idx += kBlock) {
        const int i = idx / kMaxBasis, j = idx % kMaxBasis;
        sm.T[idx] = i == j && i < p ? sm.theta[i] : 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    st->jc = p;
    st->restarts += 1;
    st->decision = UNDECIDED;
    st->open = 1;
}

// NOT_FINITE: every value and residual NaN, every vector zero
__global__ __launch_bounds__(kBlock)
void eigs_fill_failed(long long n, int k, float* __restrict__ d_values, float* __restrict__ d_residuals,
                      float* __restrict__ out, long long ldo) {
    const float nan = __builtin_nanf("");
    if (blockIdx.x == 0 && threadIdx.x < k) {
        d_values[threadIdx.x] = nan;
        if (d_residuals) d_residuals[threadIdx.x] = nan;
    }
    for (long long e = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; e < n;
         e += static_cast<long long>(gridDim.x) * kBlock) {
        for (int i = 0; i < k; ++i) out[i * ldo + e] = 0.0f;
    }
}

EigsResult solve(const CSRMatrix* A, float* d_values, float* d_vectors, long long ldv, float* d_residuals,
                 const float* d_v0, const EigsConfig* config) {
    EigsResult result;
    const auto fail = [&result](SpMVError e) {
        result.error_code = code(e);
        return result;
    };
    const EigsConfig defaults;
    const EigsConfig& cfg = config ? *config : defaults;
    int m = 0;
    bool nothing_to_do = false;
    const int status = eigs_check_arguments(A, d_values, d_vectors, ldv, d_residuals, d_v0, cfg, &m, &nothing_to_do);
    if (status != 0 || nothing_to_do) {
        result.error_code = status;
        return result;
    }
    const int n = A->num_rows;
    const int k = cfg.num_values;
    const int max_it = cfg.max_iterations;

    const TraceRange range("spmv:eigs_sym");
    hipStream_t stream = current_stream();
    TiledEngine engine(A, cfg.engine, stream);

    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / n);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const int rgrid = capped_grid(n, kBlock);
    const int ogrid = static_cast<int>(std::min<long long>((static_cast<long long>(n) + kChunk - 1) / kChunk,
                                                           kOrthoBlocks));
    // the basis: m + 1 vectors, leading dimension a multiple of 256 bytes; then w.  Every vector starts on a
    // 256-byte boundary.
    const size_t ld = (static_cast<size_t>(n) + 63) / 64 * 64;
    const size_t basis_floats = static_cast<size_t>(m + 1) * ld;
    const size_t col_count = static_cast<size_t>(kMaxBasis) * ogrid;
    const size_t res_count = 2 * static_cast<size_t>(k) * vgrid;
    Workspace<EigsState> ws;
    if (!ws.allocate(basis_floats + ld, 2 * col_count + ogrid + res_count + kSmallDoubles)) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    float* V = ws.vec;
    float* w = V + basis_floats;
    double* part1 = ws.part;
    double* part2 = part1 + col_count;
    double* ww_part = part2 + col_count;
    double* res_part = ww_part + ogrid;
    Small sm;
    sm.T = res_part + res_count;
    sm.S = sm.T + kMaxBasis * kMaxBasis;
    sm.theta = sm.S + kMaxBasis * kMaxBasis;
    sm.C = reinterpret_cast<float*>(sm.theta + kMaxBasis);
    sm.theta32 = sm.C + kMaxBasis * kMaxBasis;
    sm.h1 = sm.theta32 + kMaxBasis;
    sm.h2 = sm.h1 + kMaxBasis;
    const long long lld = static_cast<long long>(ld);

    const auto direct_spmv = [&](auto finishing, const float* in, float* out, int pair) -> bool {
        return with_lanes(lanes, [&](auto L) {
            eigs_spmv<decltype(L)::value, decltype(finishing)::value><<<row_grid, kBlock, 0, stream>>>(
                n, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, in, out, pair, ws.state);
            return hipGetLastError();
        }) == hipSuccess;
    };
    const auto step = [&](int j) -> bool {
        const float* vj = V + static_cast<size_t>(j) * ld;
        const TiledEngine::Spmv spmv = engine.spmv(vj, w, stream);
        if (spmv == TiledEngine::Spmv::FAILED) return false;
        if (spmv == TiledEngine::Spmv::DIRECT && !direct_spmv(std::false_type{}, vj, w, 0)) return false;
        eigs_multidot<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part1);
        eigs_update_multidot<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part1, sm.h1, part2);
        eigs_update_norm<<<ogrid, kBlock, 0, stream>>>(n, lld, j, V, w, ws.state, part2, sm.h2, ww_part);
        eigs_column<<<1, kBlock, 0, stream>>>(j, m, n, max_it, ww_part, ogrid, sm, ws.state);
        eigs_normalize<<<vgrid, kBlock, 0, stream>>>(n, j + 1, w, V + static_cast<size_t>(j + 1) * ld, ws.state);
        return hipGetLastError() == hipSuccess;
    };
    const auto finish = [&]() -> bool {
        eigs_rotate<true><<<rgrid, kBlock, 0, stream>>>(n, lld, V, sm.C, ws.state, d_vectors, ldv, k);
        if (hipGetLastError() != hipSuccess) return false;
        for (int i = 0; i < k; ++i) {
            const float* y = d_vectors + static_cast<long long>(i) * ldv;
            if (!direct_spmv(std::true_type{}, y, w, i)) return false;
            eigs_residual_partials<<<vgrid, kBlock, 0, stream>>>(n, w, y, i, sm.theta32, ws.state,
                                                                 res_part + 2LL * i * vgrid);
        }
        eigs_verdict<<<1, kBlock, 0, stream>>>(k, cfg.tolerance, max_it, res_part, vgrid, sm, d_values, d_residuals,
                                               ws.state);
        return hipGetLastError() == hipSuccess;
    };
    const auto restart = [&]() -> bool {
        eigs_rotate<false><<<rgrid, kBlock, 0, stream>>>(n, lld, V, sm.C, ws.state, nullptr, 0, k);
        eigs_restart<<<1, kBlock, 0, stream>>>(sm, ws.state);
        return hipGetLastError() == hipSuccess;
    };

    // setup: the start vector, its norm, v_0; one read-back
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(EigsState), stream) == hipSuccess;
    const float* start = d_v0;
    if (!start) {
        ok = ok && gen_vector(kEigsStartSeed, kEigsStartTag, static_cast<size_t>(n), w, stream) == 0;
        start = w;
    }
    if (ok) {
        eigs_norm_partials<<<vgrid, kBlock, 0, stream>>>(n, start, res_part);
        eigs_start<<<1, kBlock, 0, stream>>>(res_part, vgrid, max_it, ws.state);
        eigs_normalize<<<vgrid, kBlock, 0, stream>>>(n, 0, start, V, ws.state);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
    if (ws.pinned[0].bad_start) return fail(SpMVError::INVALID_ARGUMENT);

    if (!ws.pinned[0].done) {
        EventPair& ev = thread_events();
        ok = hipEventRecord(ev.start, stream) == hipSuccess;
        // The host follows the device's column j and step count.  A cycle that closes where the host expects it
        // (j + 1 == m, the step count reaches max_iterations) gets its close at once; one that closes early (an
        // invariant space, a value that is not finite) shows in the mirror one step late: the step enqueued in
        // between was a no-op.  Every close is a blocking read-back of the decision.  Every cycle commits a column
        // or ends the call, so max_iterations + 2 closes bound the loop.
        int j = 0;
        long long steps = 0, published = 0;
        int since_close = 0;
        bool need_close = max_it == 0;
        const long long bound = 2LL * max_it + 4;
        for (long long it = 0; ok && it < bound; ++it) {
            if (!need_close) {
                if (!engine.build_if_due(published, ws, stream, ok)) break;
                const TraceRange step_range("spmv:eigs_step");
                ok = ok && step(j);
                ++steps;
                need_close = j + 1 == m || steps >= max_it;
                ++j;
                if (ok && since_close >= 1) {
                    const EigsState* seen = ws.wait_previous(published);
                    ok = seen != nullptr;
                    if (ok && !seen->open) need_close = true;       // closed early: the step just enqueued did nothing
                }
                ok = ok && ws.publish(published, sizeof(EigsState), stream);
                ++published;
                ++since_close;
                if (!need_close) continue;
            }
            const TraceRange close_range("spmv:eigs_close");
            eigs_ritz<<<1, kBlock, 0, stream>>>(k, cfg.which, m, max_it, cfg.tolerance, sm, ws.state);
            ok = ok && hipGetLastError() == hipSuccess;
            if (!ws.read_back(ok, stream)) return fail(SpMVError::KERNEL_LAUNCH);
            if (ws.pinned[0].done) break;
            if (ws.pinned[0].decision == FINISH) {
                if (!ws.read_back(finish(), stream)) return fail(SpMVError::KERNEL_LAUNCH);
                if (ws.pinned[0].done) break;
            }
            ok = restart();
            j = ws.pinned[0].p;
            steps = ws.pinned[0].iterations;
            need_close = false;
            since_close = 0;
        }
        if (!ws.finish_timed(ok, ev, stream, &result.elapsed_ms)) return fail(SpMVError::KERNEL_LAUNCH);
    }
    const EigsState final_state = ws.pinned[0];
    if (final_state.breakdown == EigsResult::NOT_FINITE) {
        eigs_fill_failed<<<rgrid, kBlock, 0, stream>>>(n, k, d_values, d_residuals, d_vectors, ldv);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::KERNEL_LAUNCH);
        }
    }
    result.iterations = final_state.iterations;
    result.restarts = final_state.restarts;
    result.converged = final_state.breakdown == EigsResult::NOT_FINITE ? 0 : final_state.converged;
    result.breakdown = final_state.breakdown;
    result.max_residual = final_state.breakdown == EigsResult::NOT_FINITE
                              ? std::numeric_limits<float>::quiet_NaN()
                              : static_cast<float>(final_state.max_residual);
    return result;
}

} // namespace
} // namespace detail

EigsResult eigs_sym(const CSRMatrix* A, float* d_values, float* d_vectors, long long ldv, float* d_residuals,
                    const float* d_v0, const EigsConfig* config) {
    return detail::solve(A, d_values, d_vectors, ldv, d_residuals, d_v0, config);
}

int sym_eig_small(int n, const double* T, int ld, double* values, double* vectors, int on_device) {
    using namespace detail;
    using namespace detail::eigs;
    bool nothing_to_do = false;
    const int status = sym_eig_small_check(n, T, ld, values, vectors, &nothing_to_do);
    if (status != 0 || nothing_to_do) return status;
    if (!on_device) {
        sym_eig_small_host(n, T, ld, values, vectors);
        return 0;
    }
    constexpr int kOrder = kMaxOrder;
    hipStream_t stream = current_stream();
    DevBuf<double> buf;          // T, S, vectors (kOrder x kOrder each), values
    if (dev_alloc(&buf, 3LL * kOrder * kOrder + kOrder) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    double* d_T = buf.get();
    double* d_S = d_T + kOrder * kOrder;
    double* d_vec = d_S + kOrder * kOrder;
    double* d_val = d_vec + kOrder * kOrder;
    std::vector<double> packed(static_cast<size_t>(kOrder) * kOrder, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) packed[static_cast<size_t>(i) * kOrder + j] = T[static_cast<size_t>(i) * ld + j];
    }
    bool ok = hipMemcpyAsync(d_T, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, stream) ==
              hipSuccess;
    if (ok) {
        sym_eig_small_kernel<<<1, dev::kBlock, 0, stream>>>(n, d_T, d_S, d_val, d_vec);
        ok = hipGetLastError() == hipSuccess;
    }
    std::vector<double> out_values(kOrder);
    ok = ok && hipMemcpyAsync(packed.data(), d_vec, packed.size() * sizeof(double), hipMemcpyDeviceToHost, stream) ==
                   hipSuccess &&
         hipMemcpyAsync(out_values.data(), d_val, kOrder * sizeof(double), hipMemcpyDeviceToHost, stream) ==
             hipSuccess &&
         hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    for (int i = 0; i < n; ++i) {
        values[i] = out_values[i];
        for (int l = 0; l < n; ++l) vectors[static_cast<size_t>(i) * ld + l] = packed[static_cast<size_t>(i) * kOrder + l];
    }
    return 0;
}

} // namespace spmv
