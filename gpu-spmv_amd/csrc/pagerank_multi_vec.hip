// pagerank_multi_vec.hip — personalized PageRank for k teleport vectors in one matrix pass per step
// (include/spmv/pagerank.h pagerank_personalized).
//
// pagerank.hip's direct-engine loop, k-wide: V (the teleport distributions) and R are num_rows x k row-major; the
// loop keeps its own copy of V and two rank arrays, each cut into windows of W = 4 (k <= 4) or 8 columns, a window
// being a num_rows x W row-major array of its own (a pass over one window streams whole lines and every row slice is
// 16-byte aligned).  Every column has its own device state (PprColumn) and its own partials; a header in front of
// the column states carries the global `done` the host polls.  Per step, two launches whatever k:
//   ppr_step_kernel<LANES, W, NW>  per column: r_new = d (A r_old) + (d s) v + (1 - d) v, the block partials of
//                                  ||r_new - r_old||^2 and of the dangling mass of r_new
//   ppr_commit_kernel<W>           one workgroup, per column: the fold, residual, iteration count, next dangling mass,
//                                  the stop test and the buffer the column was last written to; then the global flag
// Column j is bit for bit the k = 1 call on V[:, j], and for V[:, j] = 1/n with n a power of two it is pagerank() on
// the direct kernels: a row's sum is row_partial_dot<LANES>'s walk with one accumulator per column, the
// thread-to-row mapping and the grid are pr_step_kernel's, and each column's partials are laid out and folded as
// pr_step_kernel / pr_fold_and_commit lay out and fold theirs.  A column that is done is frozen: no kernel writes its
// ranks or state again, so columns frozen at different step parities rest in different buffers until the final
// normalise (pr_normalise's blocks and fold, per column) gathers them into d_R.  No float atomics, no waiting between
// workgroups.
#include "internal.h"
#include "device_common.h"
#include "multi_window.h"
#include "pagerank_engine.h"
#include "solver_common.h"
#include "spmv/pagerank.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using namespace dev;
using namespace solver;

constexpr int kMaxColumns = 32;
constexpr int kNormaliseBlocks = 1024;        // pr_normalise's

// pagerank_engine.h's PrState, one per column.
struct PprColumn {
    float dangling_sum;       // dangling mass of the column's current ranks
    float final_residual;     // ||r_new - r_old||_2 of its last committed step
    int   iterations;         // committed steps
    int   converged;
    int   done;               // frozen: nothing of this column is written again
    int   parity;             // which of the two rank arrays holds its last committed ranks
    int   bad;                // setup: a negative or non-finite entry, or a sum that is not > 0
    int   reserved;
};

struct PprState {
    int done;                 // every column is done: steps after this are no-ops
    int bad;                  // some column of V was refused
    unsigned bad_entries;     // bit j: column j of V holds a negative or non-finite entry
    int reserved;
    PprColumn col[kMaxColumns];
};

constexpr size_t kHeaderBytes = offsetof(PprState, col);

// Setup, a thread per row of V: refuses negative and non-finite entries (bit j of state->bad_entries), copies V into
// the loop's windows (vw, and r0 = the start vector; padding columns 0) and leaves per column the block partials of
// the column sum and of its dangling mass -> part[(2 * gridDim.x) * column + 2 * block].
template <int W>
__global__ __launch_bounds__(kBlock)
void ppr_setup_kernel(int n, int k, const float* __restrict__ V, long long ldv, bool v_vec,
                      const unsigned char* __restrict__ dangling, float* __restrict__ vw, float* __restrict__ r0,
                      PprState* __restrict__ state, double* __restrict__ part) {
    const long long out_stride = 2LL * gridDim.x;
    unsigned bad = 0;
    for (int j0 = 0; j0 < k; j0 += W) {
        const long long window = static_cast<long long>(j0 / W) * n * W;
        double sums[2 * W];           // sum, dangling mass of column j0 + c at [2 * c ..]
#pragma unroll
        for (int c = 0; c < 2 * W; ++c) sums[c] = 0.0;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float v[W];
            load_window<W>(V, ldv, i, j0, k, v_vec, v);
            const bool dang = dangling[i] != 0;
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (!(v[c] >= 0.0f) || v[c] > 3.402823466e38f) bad |= 1u << (j0 + c);     // negative, NaN, inf
                sums[2 * c] += static_cast<double>(v[c]);
                if (dang) sums[2 * c + 1] += static_cast<double>(v[c]);
            }
            store_own<W>(vw + window, i, v);
            store_own<W>(r0 + window, i, v);
        }
        const double total = block_sum_columns<2 * W>(sums);
        const int c = threadIdx.x / 2;
        if (c < W && j0 + c < k) part[out_stride * (j0 + c) + 2LL * blockIdx.x + threadIdx.x % 2] = total;
    }
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicOr(&state->bad_entries, bad);
}

// One workgroup: per column the fold of the setup partials, the verdict on V[:, j] and the starting dangling mass.
__global__ __launch_bounds__(kBlock)
void ppr_start_kernel(const double* __restrict__ part, int count, int k, PprState* __restrict__ state) {
    int refused = 0;
    for (int j = 0; j < k; ++j) {
        double sum = 0.0, mass = 0.0;
        fold_partials(part + 2LL * count * j, count, 2, sum, mass);
        if (threadIdx.x != 0) continue;
        PprColumn& c = state->col[j];
        c.dangling_sum = static_cast<float>(mass);
        if (((state->bad_entries >> j) & 1u) || !(sum > 0.0)) {
            c.bad = 1;
            ++refused;
        }
    }
    if (threadIdx.x == 0 && refused) {
        state->bad = 1;
        state->done = 1;
    }
}

// The columns still running (bit j), the same in every thread of the workgroup, and d * s of every column in LDS.
// 0 once the global flag is up.  Nothing in a step launch writes the state, so every workgroup sees the same.
__device__ __forceinline__ unsigned step_prologue(const PprState* __restrict__ state, int k, float damping,
                                                  float (&dterm)[kMaxColumns]) {
    __shared__ unsigned s_active;
    if (threadIdx.x == 0) {
        unsigned a = 0;
        if (!state->done) {
            for (int j = 0; j < k; ++j) a |= state->col[j].done ? 0u : 1u << j;
        }
        s_active = a;
    }
    if (threadIdx.x < kMaxColumns) {
        dterm[threadIdx.x] = threadIdx.x < k ? __fmul_rn(damping, state->col[threadIdx.x].dangling_sum) : 0.0f;
    }
    __syncthreads();
    return s_active;
}

// One power-iteration step of every running column.  A workgroup takes the NW windows of W columns from window
// blockIdx.y * NW on, inside the row loop: the row's entries come from cache after the first window.  (k > 16 runs
// as two such groups side by side in one launch, gridDim.y = 2: four windows in one workgroup need 64 fp64 sums per
// thread and leave one wavefront per SIMD.)  A window of frozen columns is not walked; a frozen column inside a
// running window rides along in the gather and nothing of it is stored.  Block partials -> part[part_stride * column
// + 2 * blockIdx.x] (residual^2, dangling mass).
template <int LANES, int W, int NW>
__global__ __launch_bounds__(kBlock)
void ppr_step_kernel(int n, long long nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                     const float* __restrict__ vals, const float* __restrict__ r_old, float* __restrict__ r_new,
                     const float* __restrict__ vw, const unsigned char* __restrict__ dangling, float damping, int k,
                     const PprState* __restrict__ state, double* __restrict__ part, long long part_stride) {
    __shared__ float s_dterm[kMaxColumns];
    const int first_column = blockIdx.y * NW * W;
    const unsigned active = (step_prologue(state, k, damping, s_dterm) >> first_column) & ((1u << NW * W) - 1u);
    if (!active) return;
    constexpr int kRowsPerBlock = kBlock / LANES;
    constexpr unsigned kWindowMask = W == 32 ? 0xffffffffu : (1u << W) - 1u;
    const long long window = static_cast<long long>(n) * W;      // floats of one window
    const long long group = static_cast<long long>(blockIdx.y) * NW * window;
    r_old += group;
    r_new += group;
    vw += group;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    const float teleport = __fsub_rn(1.0f, damping);
    double sums[2 * NW * W];          // residual^2, dangling mass of column first_column + c at [2 * c ..]
#pragma unroll
    for (int c = 0; c < 2 * NW * W; ++c) sums[c] = 0.0;
    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < n;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long row = first + slot;
        const int begin = row < n ? row_ptrs[row] : 0;
        const int end = row < n ? row_ptrs[row + 1] : 0;
#pragma unroll
        for (int wi = 0; wi < NW; ++wi) {
            const int j0 = wi * W;
            const unsigned m = (active >> j0) & kWindowMask;     // (no bit at or past column k is ever set)
            if (!m) continue;
            const float* old_w = r_old + wi * window;
            float acc[W];
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] = 0.0f;
            if (row < n) {
                row_partial_dot_multi<LANES, W, true>(begin, end, lane, nnz, cols, vals, old_w, W, 0, 0, true, acc);
            }
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] = group_sum<LANES>(acc[c]);
            if (lane == 0 && row < n) {
                float v[W], old[W], fresh[W];
                load_own<W>(vw + wi * window, W, row, 0, v);
                load_own<W>(old_w, W, row, 0, old);
                const bool dang = dangling[row] != 0;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    // pr_step_kernel's expression order: d * y + (d * s) * v + (1 - d) * v
                    fresh[c] = __fadd_rn(__fadd_rn(__fmul_rn(damping, acc[c]), __fmul_rn(s_dterm[first_column + j0 + c], v[c])),
                                         __fmul_rn(teleport, v[c]));
                    const float diff = __fsub_rn(fresh[c], old[c]);
                    sums[2 * (j0 + c)] += static_cast<double>(__fmul_rn(diff, diff));
                    if (dang) sums[2 * (j0 + c) + 1] += static_cast<double>(fresh[c]);
                }
                float* new_w = r_new + wi * window;
                if (m == kWindowMask) {
                    store_own<W>(new_w, row, fresh);
                } else {
#pragma unroll
                    for (int c = 0; c < W; ++c) {
                        if ((m >> c) & 1u) new_w[row * W + c] = fresh[c];
                    }
                }
            }
        }
    }
    const double total = block_sum_columns<2 * NW * W>(sums);
    const int c = threadIdx.x / 2;
    if (c < NW * W && ((active >> c) & 1u)) {
        part[part_stride * (first_column + c) + 2LL * blockIdx.x + threadIdx.x % 2] = total;
    }
}

// One workgroup: pr_fold_and_commit per running column (W columns' folds at once), then the global flag.  `step` is
// the 0-based step whose partials these are: it wrote rank array (step + 1) & 1.
template <int W>
__global__ __launch_bounds__(kBlock)
void ppr_commit_kernel(const double* __restrict__ part, int count, long long part_stride, int k, int step,
                       float tolerance, PprState* __restrict__ state) {
    if (state->done) return;
    int finished = 0;                 // thread 0's count
    for (int j0 = 0; j0 < k; j0 += W) {
        unsigned running = 0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (j0 + c < k && !state->col[j0 + c].done) running |= 1u << c;
        }
        finished += min(W, k - j0) - __popc(running);
        if (!running) continue;
        double sums[2 * W];
#pragma unroll
        for (int c = 0; c < 2 * W; ++c) sums[c] = 0.0;
        for (int b = threadIdx.x; b < count; b += kBlock) {
#pragma unroll
            for (int c = 0; c < W; ++c) {             // (all W: the array is padded to whole windows)
                const double* mine = part + part_stride * (j0 + c) + 2LL * b;
                sums[2 * c] += mine[0];
                sums[2 * c + 1] += mine[1];
            }
        }
        fold_values<2 * W>(sums);
        if (threadIdx.x != 0) continue;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (!((running >> c) & 1u)) continue;
            PprColumn& col = state->col[j0 + c];
            const float residual = static_cast<float>(sqrt(sums[2 * c]));
            col.iterations = step + 1;
            col.final_residual = residual;
            col.dangling_sum = static_cast<float>(sums[2 * c + 1]);
            col.parity = (step + 1) & 1;
            if (residual < tolerance) {
                col.converged = 1;
                col.done = 1;
                ++finished;
            }
        }
    }
    if (threadIdx.x == 0 && finished == k) state->done = 1;
}

// Row i of window `window_offset` as the columns were last committed: column c from r0 or r1 by its parity bit.
template <int W>
__device__ __forceinline__ void load_committed(const float* __restrict__ r0, const float* __restrict__ r1,
                                               long long window_offset, long long row, unsigned parity,
                                               float (&out)[W]) {
    float a[W], b[W];
    load_own<W>(r0 + window_offset, W, row, 0, a);
    load_own<W>(r1 + window_offset, W, row, 0, b);
#pragma unroll
    for (int c = 0; c < W; ++c) out[c] = (parity >> c) & 1u ? b[c] : a[c];
}

__device__ __forceinline__ unsigned committed_parities(const PprState* __restrict__ state, int k) {
    __shared__ unsigned s_parity;
    if (threadIdx.x == 0) {
        unsigned p = 0;
        for (int j = 0; j < k; ++j) p |= state->col[j].parity ? 1u << j : 0u;
        s_parity = p;
    }
    __syncthreads();
    return s_parity;
}

// pr_vector_sum_kernel per column -> block_out[gridDim.x * column + block]
template <int W>
__global__ __launch_bounds__(kBlock)
void ppr_sum_kernel(int n, int k, const float* __restrict__ r0, const float* __restrict__ r1,
                    const PprState* __restrict__ state, double* __restrict__ block_out) {
    const unsigned parity = committed_parities(state, k);
    for (int j0 = 0; j0 < k; j0 += W) {
        const long long window = static_cast<long long>(j0 / W) * n * W;
        double acc[W];
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = 0.0;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float v[W];
            load_committed<W>(r0, r1, window, i, parity >> j0, v);
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] += static_cast<double>(v[c]);
        }
        const double total = block_sum_columns<W>(acc);
        const int c = threadIdx.x;
        if (c < W && j0 + c < k) block_out[static_cast<long long>(gridDim.x) * (j0 + c) + blockIdx.x] = total;
    }
}

// pr_scale_kernel per column, into the caller's R: R[i, j] = r_j[i] / sum(r_j) (as it is where the sum is not > 0)
template <int W>
__global__ __launch_bounds__(kBlock)
void ppr_scale_kernel(int n, int k, const float* __restrict__ r0, const float* __restrict__ r1,
                      const PprState* __restrict__ state, const double* __restrict__ block_sums, int blocks,
                      float* __restrict__ R, long long ldr) {
    __shared__ float s_total[kMaxColumns];
    if (threadIdx.x < k) {
        double total = 0.0;
        for (int b = 0; b < blocks; ++b) total += block_sums[static_cast<long long>(blocks) * threadIdx.x + b];
        s_total[threadIdx.x] = static_cast<float>(total);
    }
    const unsigned parity = committed_parities(state, k);      // (its barrier publishes s_total too)
    for (int j0 = 0; j0 < k; j0 += W) {
        const long long window = static_cast<long long>(j0 / W) * n * W;
        for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
             i += static_cast<long long>(gridDim.x) * kBlock) {
            float v[W];
            load_committed<W>(r0, r1, window, i, parity >> j0, v);
#pragma unroll
            for (int c = 0; c < W; ++c) {
                if (j0 + c < k) {
                    const float total = s_total[j0 + c];
                    R[i * ldr + j0 + c] = total > 0.0f ? __fdiv_rn(v[c], total) : v[c];
                }
            }
        }
    }
}

// V[node, j] = 1 / |set j| for every listed node; V (num_rows x k, ld = k) was zeroed before.
__global__ __launch_bounds__(kBlock)
void ppr_seed_fill_kernel(const int* __restrict__ seed_ptrs, const int* __restrict__ seed_nodes, int k,
                          float* __restrict__ V) {
    const int first = seed_ptrs[0], total = seed_ptrs[k] - first;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < total; idx += gridDim.x * kBlock) {
        int j = 0;
        while (seed_ptrs[j + 1] <= first + idx) ++j;
        const float value = __fdiv_rn(1.0f, static_cast<float>(seed_ptrs[j + 1] - seed_ptrs[j]));
        V[static_cast<long long>(seed_nodes[first + idx]) * k + j] = value;
    }
}

template <int LANES, int W, int NW>
hipError_t launch_step(const CSRMatrix* A, const float* r_old, float* r_new, const float* vw,
                       const unsigned char* dangling, float damping, int k, const PprState* state, double* part,
                       int grid, hipStream_t s) {
    const dim3 blocks(grid, (k + NW * W - 1) / (NW * W));
    ppr_step_kernel<LANES, W, NW><<<blocks, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices,
                                                          A->d_values, r_old, r_new, vw, dangling, damping, k, state,
                                                          part, 2LL * grid);
    return hipGetLastError();
}

// windows: one of 4 columns up to k = 4, then 1 or 2 of 8 columns, then two groups of 2
hipError_t step(int lanes, const CSRMatrix* A, const float* r_old, float* r_new, const float* vw,
                const unsigned char* dangling, float damping, int k, const PprState* state, double* part, int grid,
                hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        constexpr int kLanes = decltype(L)::value;
        if (k <= 4) return launch_step<kLanes, 4, 1>(A, r_old, r_new, vw, dangling, damping, k, state, part, grid, s);
        if (k <= 8) return launch_step<kLanes, 8, 1>(A, r_old, r_new, vw, dangling, damping, k, state, part, grid, s);
        return launch_step<kLanes, 8, 2>(A, r_old, r_new, vw, dangling, damping, k, state, part, grid, s);
    });
}

// the floats [a, a + na) and [b, b + nb) share a byte
bool spans_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) &&
           b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

// pagerank()'s dangling mask, computed the way pagerank() computes it without a plan: the reference's sequential
// fp32 column sums in storage order where the host arrays exist, else atomic column sums on the device.  Computed
// per call into the call's own memory: pagerank()'s cached copy belongs to whichever pagerank() call holds the
// matrix's workspace, and this call neither reads nor writes that workspace.
bool dangling_mask(const CSRMatrix* A, unsigned char* d_mask, hipStream_t stream) {
    const int n = A->num_rows;
    if (hipMemsetAsync(d_mask, 0, static_cast<size_t>(n), stream) != hipSuccess) return false;
    if (A->values && A->col_indices && A->row_ptrs) {
        std::vector<float> sums(static_cast<size_t>(n), 0.0f);
        for (int r = 0; r < n; ++r) {
            for (int j = A->row_ptrs[r]; j < A->row_ptrs[r + 1]; ++j) {
                const int c = A->col_indices[j];
                if (c >= 0 && c < n) sums[c] += A->values[j];
            }
        }
        std::vector<unsigned char> mask(static_cast<size_t>(n));
        for (int c = 0; c < n; ++c) mask[c] = sums[c] == 0.0f;
        return hipMemcpyAsync(d_mask, mask.data(), mask.size(), hipMemcpyHostToDevice, stream) == hipSuccess
            && hipStreamSynchronize(stream) == hipSuccess;
    }
    DevBuf<float> col_sums;
    DevBuf<unsigned long long> count;
    return dev_alloc(&col_sums, n) == hipSuccess && dev_alloc(&count, 1) == hipSuccess
        && hipMemsetAsync(col_sums.get(), 0, static_cast<size_t>(n) * sizeof(float), stream) == hipSuccess
        && hipMemsetAsync(count.get(), 0, sizeof(unsigned long long), stream) == hipSuccess
        && pr_column_sums(A->nnz, A->d_col_indices, A->d_values, n, col_sums.get(), stream) == hipSuccess
        && pr_mask_from_column_sums(col_sums.get(), n, d_mask, count.get(), stream) == hipSuccess
        && hipStreamSynchronize(stream) == hipSuccess;
}

int ppr_lanes_for(const CSRMatrix* A) {
    if (int f = forced_lanes("ppr_lanes")) return f;
    return pick_lanes_per_row(static_cast<float>(A->nnz) / A->num_rows);
}

// Checks 1 - 7 of pagerank.h (everything but the overlap); *nothing_to_do: the graph has no nodes (results written).
int check_arguments(const CSRMatrix* adj, const void* teleport, int ldv, const float* d_R, int ldr, int k,
                    const PageRankConfig* config, PersonalizedResult* results, bool* nothing_to_do) {
    *nothing_to_do = false;
    const auto fail = [&](SpMVError e) {
        if (results && k >= 1 && k <= kMaxColumns) {       // a k out of range says nothing about the array's length
            for (int j = 0; j < k; ++j) results[j].error_code = code(e);
        }
        return code(e);
    };
    if (!adj || !teleport || !d_R || !results) return fail(SpMVError::INVALID_ARGUMENT);
    if (k < 1 || k > kMaxColumns) return fail(SpMVError::INVALID_ARGUMENT);
    if (ldv < k || ldr < k) return fail(SpMVError::INVALID_ARGUMENT);
    if (adj->num_rows != adj->num_cols) return fail(SpMVError::INVALID_DIMENSION);
    if (adj->num_rows == 0) {
        for (int j = 0; j < k; ++j) {
            results[j] = PersonalizedResult{code(SpMVError::SUCCESS), 0, 0.0f, 1, 0.0f};
        }
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (!device_arrays_strict(adj)) return fail(SpMVError::INVALID_FORMAT);
    if (config) {
        const float d = config->damping_factor, tol = config->tolerance;
        if (!(d > 0.0f && d < 1.0f) || !(tol >= 0.0f) || std::isinf(tol) || config->max_iterations < 0) {
            return fail(SpMVError::INVALID_ARGUMENT);
        }
    }
    return code(SpMVError::SUCCESS);
}

int personalized(const CSRMatrix* adj, const float* d_V, int ldv, float* d_R, int ldr, int k,
                 const PageRankConfig* config, PersonalizedResult* results) {
    bool nothing_to_do = false;
    const int checked = check_arguments(adj, d_V, ldv, d_R, ldr, k, config, results, &nothing_to_do);
    if (checked != code(SpMVError::SUCCESS) || nothing_to_do) return checked;
    const auto fail = [&](SpMVError e) {
        for (int j = 0; j < k; ++j) results[j].error_code = code(e);
        return code(e);
    };
    const int n = adj->num_rows;
    if (spans_overlap(d_V, static_cast<long long>(n - 1) * ldv + k, d_R, static_cast<long long>(n - 1) * ldr + k)) {
        return fail(SpMVError::INVALID_ARGUMENT);
    }
    const PageRankConfig defaults;
    const PageRankConfig& cfg = config ? *config : defaults;

    const TraceRange range("spmv:pagerank_personalized");
    hipStream_t stream = current_stream();

    const int lanes = ppr_lanes_for(adj);
    const int row_grid = capped_grid(n, kBlock / lanes);
    const int vgrid = vec_grid(n);
    const int nblocks = static_cast<int>(std::min<long long>(kNormaliseBlocks, (static_cast<long long>(n) + kBlock - 1) / kBlock));
    const int w = k <= 4 ? 4 : 8;
    const size_t k_pad = static_cast<size_t>((k + w - 1) / w * w);      // whole windows: the folds read all W columns of one
    const size_t len = static_cast<size_t>(n) * k_pad;
    const size_t part_count = k_pad * 2 * static_cast<size_t>(std::max({row_grid, vgrid, nblocks}));

    Workspace<PprState> ws;           // the two rank arrays and the copy of V, ceil(k / w) windows of n x w each
    DevBuf<unsigned char> mask;
    if (!ws.allocate(3 * len, part_count) || dev_alloc(&mask, n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SpMVError::CUDA_MALLOC);
    }
    float* bufs[2] = {ws.vec, ws.vec + len};
    float* vw = ws.vec + 2 * len;
    PprState* pinned = ws.pinned;
    const bool v_vec = ldv % 4 == 0 && (reinterpret_cast<uintptr_t>(d_V) & 15) == 0;

    // setup: the mask, the windows, every column's verdict and starting dangling mass; one read-back
    bool ok = dangling_mask(adj, mask.get(), stream)
           && hipMemsetAsync(ws.state, 0, sizeof(PprState), stream) == hipSuccess;
    if (ok) {
        ok = with_window(w, [&](auto W) {
            ppr_setup_kernel<decltype(W)::value><<<vgrid, kBlock, 0, stream>>>(n, k, d_V, ldv, v_vec, mask.get(), vw,
                                                                               bufs[0], ws.state, ws.part);
            ppr_start_kernel<<<1, kBlock, 0, stream>>>(ws.part, vgrid, k, ws.state);
            return hipGetLastError();
        }) == hipSuccess;
    }
    if (!ws.read_back(ok, stream, kHeaderBytes)) return fail(SpMVError::KERNEL_LAUNCH);
    if (pinned[0].bad) return fail(SpMVError::INVALID_ARGUMENT);

    float elapsed_ms = 0.0f;
    EventPair& ev = thread_events();
    const bool run_loop = cfg.max_iterations > 0;
    if (run_loop) ok = hipEventRecord(ev.start, stream) == hipSuccess;
    for (int iter = 0; ok && iter < cfg.max_iterations; ++iter) {
        const TraceRange step_range("spmv:pagerank_personalized_step");
        ok = step(lanes, adj, bufs[iter & 1], bufs[(iter + 1) & 1], vw, mask.get(), cfg.damping_factor, k, ws.state,
                  ws.part, row_grid, stream) == hipSuccess;
        if (ok) {
            // the host needs the global flag alone per step: the header in front of the column states
            ok = with_window(w, [&](auto W) {
                ppr_commit_kernel<decltype(W)::value><<<1, kBlock, 0, stream>>>(ws.part, row_grid, 2LL * row_grid, k,
                                                                               iter, cfg.tolerance, ws.state);
                return hipGetLastError();
            }) == hipSuccess && ws.publish(iter, kHeaderBytes, stream);
        }
        if (ok && iter >= 1) {
            const PprState* seen = ws.wait_previous(iter);
            ok = seen != nullptr;
            if (ok && seen->done) break;
        }
    }
    if (ok && run_loop) ok = hipEventRecord(ev.stop, stream) == hipSuccess;
    if (ok) {
        // every column from the rank array it was last committed to, divided by its sum, into the caller's R
        const hipError_t e = with_window(w, [&](auto WC) {
            constexpr int W = decltype(WC)::value;
            ppr_sum_kernel<W><<<nblocks, kBlock, 0, stream>>>(n, k, bufs[0], bufs[1], ws.state, ws.part);
            ppr_scale_kernel<W><<<nblocks, kBlock, 0, stream>>>(n, k, bufs[0], bufs[1], ws.state, ws.part, nblocks, d_R,
                                                                ldr);
            return hipGetLastError();
        });
        ok = ws.read_back(e == hipSuccess, stream);
        float ms = 0.0f;
        if (ok && run_loop && hipEventElapsedTime(&ms, ev.start, ev.stop) == hipSuccess) elapsed_ms = ms;
    }
    if (!ok) {
        (void)hipGetLastError();
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    for (int j = 0; j < k; ++j) {
        const PprColumn& c = pinned[0].col[j];
        results[j] = PersonalizedResult{code(SpMVError::SUCCESS), c.iterations, c.final_residual, c.converged,
                                        elapsed_ms};
    }
    return code(SpMVError::SUCCESS);
}

int personalized_seeds(const CSRMatrix* adj, const int* seed_ptrs, const int* seed_nodes, int k, float* d_R, int ldr,
                       const PageRankConfig* config, PersonalizedResult* results) {
    bool nothing_to_do = false;
    // (seed_nodes stands in for V: the sets are read only after these checks, and V is built with ld = k)
    const int checked = check_arguments(adj, seed_ptrs && seed_nodes ? static_cast<const void*>(seed_nodes) : nullptr,
                                        k, d_R, ldr, k, config, results, &nothing_to_do);
    if (checked != code(SpMVError::SUCCESS) || nothing_to_do) return checked;
    const auto fail = [&](SpMVError e) {
        for (int j = 0; j < k; ++j) results[j].error_code = code(e);
        return code(e);
    };
    const int n = adj->num_rows;
    if (seed_ptrs[0] < 0) return fail(SpMVError::INVALID_ARGUMENT);
    std::vector<int> seen(static_cast<size_t>(n), -1);      // the last set that listed the node
    for (int j = 0; j < k; ++j) {
        if (seed_ptrs[j + 1] <= seed_ptrs[j]) return fail(SpMVError::INVALID_ARGUMENT);       // an empty set
        for (int p = seed_ptrs[j]; p < seed_ptrs[j + 1]; ++p) {
            const int node = seed_nodes[p];
            if (node < 0 || node >= n || seen[node] == j) return fail(SpMVError::INVALID_ARGUMENT);
            seen[node] = j;
        }
    }
    hipStream_t stream = current_stream();
    const int first = seed_ptrs[0], total = seed_ptrs[k] - first;
    DevBuf<float> V;
    DevBuf<int> d_ptrs, d_nodes;
    if (dev_alloc(&V, static_cast<long long>(n) * k) != hipSuccess || dev_alloc(&d_ptrs, k + 1) != hipSuccess ||
        dev_alloc(&d_nodes, seed_ptrs[k]) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SpMVError::CUDA_MALLOC);
    }
    bool ok = hipMemsetAsync(V.get(), 0, static_cast<size_t>(n) * k * sizeof(float), stream) == hipSuccess
           && hipMemcpyAsync(d_ptrs.get(), seed_ptrs, (k + 1) * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess
           && hipMemcpyAsync(d_nodes.get() + first, seed_nodes + first, total * sizeof(int), hipMemcpyHostToDevice,
                             stream) == hipSuccess;
    if (ok) {
        ppr_seed_fill_kernel<<<vec_grid(total), kBlock, 0, stream>>>(d_ptrs.get(), d_nodes.get(), k, V.get());
        ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;     // the host arrays are free again
    }
    if (!ok) {
        (void)hipGetLastError();
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    return personalized(adj, V.get(), k, d_R, ldr, k, config, results);
}

} // namespace
} // namespace detail

int pagerank_personalized(const CSRMatrix* adj, const float* d_V, int ldv, float* d_R, int ldr, int k,
                          const PageRankConfig* config, PersonalizedResult* results) {
    return detail::personalized(adj, d_V, ldv, d_R, ldr, k, config, results);
}

int pagerank_personalized_seeds(const CSRMatrix* adj, const int* seed_ptrs, const int* seed_nodes, int k, float* d_R,
                                int ldr, const PageRankConfig* config, PersonalizedResult* results) {
    return detail::personalized_seeds(adj, seed_ptrs, seed_nodes, k, d_R, ldr, config, results);
}

} // namespace spmv
