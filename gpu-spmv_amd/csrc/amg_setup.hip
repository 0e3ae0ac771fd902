// amg_setup.hip — the device-side AMG setup (include/spmv/amg.h): the MIS-2 aggregation of one level
// (amg_aggregate_mis2_gpu; amg_aggregate_mis2_cpu_csr in amg_mis2_host.cpp is its definition), amg_setup_device and
// amg_update on the hierarchies it builds.
//
//   diagonal     one thread per row: d_i (fp32, storage order), wd_i = float(double(omega) / double(d_i)) and the
//                smallest row whose diagonal is missing, not > 0 or not finite, as one minimum per workgroup
//   roots        Jones-Plassmann in rounds, the host loop being csr_color's (solver::run_rounds).  A round is one
//                launch: 1-64 lanes share an undecided row v, split its strong entries and walk, for each of them,
//                the strong entries of that neighbour's row (a direct 2-hop pull from A's rows).  Priorities are
//                recomputed from the index; the strength test is re-evaluated from d on the fly.  The states
//                are updated in place: v becomes OUT when it saw a higher-priority ROOT, ROOT when every
//                higher-priority vertex it saw was OUT.  A state is written once, by one aligned 4-byte store, and
//                both rules only act on states that are final, so which of the current round's writes a vertex
//                happens to see changes the round it decides in, never its state.
//                The only atomic is one add per workgroup to the count of vertices left.
//   numbers      the root flags scanned by csr_build.hip's scan
//   phase 1, 2   lanes share a row again; phase 1 writes a second array so that phase 2 reads end-of-phase-1
//                membership; phase 2 folds (|v|, storage position) to the maximum, ties to the smaller position
//   P            row_ptrs = iota, cols = the aggregate map (phase 2 writes it in place), vals = 1
//   smoothing    amg_smooth_coarsen, the coarsening step of a smoothed hierarchy for this builder and amg_host.cpp's:
//                P = T + diag(s) (A T) through spgemm_csr, csr_scale_gpu and csr_add, then P^T and the two products
// No kernel here waits for another workgroup; none uses an atomic on a value.
#include "amg_impl.h"
#include "reorder_impl.h"
#include "solver_common.h"
#include "spmv/csr_ops.h"
#include "spmv/spgemm.h"

#include <chrono>
#include <climits>
#include <memory>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using dev::block_min;
using dev::capped_grid;
using dev::group_or;
using dev::kBlock;
using dev::vec_grid;
using dev::with_lanes;
using reorder::higher_priority;

constexpr int kUndecided = 0, kRoot = 1, kOut = 2;

// the device state of one level's setup; remaining[r % 3] = vertices still undecided after round r
struct Mis2State {
    int remaining[3];
    int rounds;          // rounds that found something to do
    int count;           // roots = aggregates
    int bad_row;         // the smallest row with a bad diagonal, or INT_MAX
    int free_row;        // the smallest row left without an aggregate, or INT_MAX
};

// min over an aligned group of LANES consecutive lanes, every lane gets the result
template <int LANES>
__device__ __forceinline__ int group_min(int v) {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

// d, wd (null: the diagonals are taken as they come, nothing is checked) and partial[b] = the smallest bad row
// workgroup b saw
__global__ __launch_bounds__(kBlock)
void amg_diag_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const float* __restrict__ va,
                     float omega, float* __restrict__ d, float* __restrict__ wd, int* __restrict__ partial) {
    int bad = INT_MAX;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float sum = 0.0f;
        bool found = false;
        const int end = rp[i + 1];
        for (int p = rp[i]; p < end; ++p) {
            if (ci[p] == i) {
                sum = __fadd_rn(sum, va[p]);
                found = true;
            }
        }
        if (d) d[i] = sum;
        if (wd) {
            if (!found || !(sum > 0.0f) || !isfinite(sum)) bad = min(bad, static_cast<int>(i));
            wd[i] = static_cast<float>(static_cast<double>(omega) / static_cast<double>(sum));
        }
    }
    bad = block_min(bad);
    if (threadIdx.x == 0) partial[blockIdx.x] = bad;
}

// *out = min(partial[0 .. count)); one workgroup
__global__ __launch_bounds__(kBlock) void min_fold_kernel(const int* __restrict__ partial, int count,
                                                          int* __restrict__ out) {
    int m = INT_MAX;
    for (int i = threadIdx.x; i < count; i += kBlock) m = min(m, partial[i]);
    m = block_min(m);
    if (threadIdx.x == 0) *out = m;
}

__global__ __launch_bounds__(kBlock) void mis2_init_kernel(int n, int* __restrict__ state, Mis2State* __restrict__ st) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        state[i] = kUndecided;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->remaining[0] = 0;
        st->remaining[1] = 0;
        st->remaining[2] = n;       // "after round -1"
        st->rounds = 0;
        st->count = 0;
        st->free_row = INT_MAX;
    }
}

// bit 0: u has a higher priority than v and is a ROOT; bit 1: ... and is undecided
__device__ __forceinline__ unsigned look(int u, int v, unsigned seed, const int* state) {
    if (!higher_priority(u, v, seed)) return 0u;
    const int s = state[u];
    return s == kRoot ? 1u : (s == kUndecided ? 2u : 0u);
}

// One round.  `state` is read and written in place (see the head of this file).
template <int LANES>
__global__ __launch_bounds__(kBlock)
void mis2_round_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const float* __restrict__ va,
                       const float* __restrict__ d, double theta2, unsigned seed, int* state, Mis2State* st,
                       int round) {
    if (st->remaining[(round + 2) % 3] == 0) {                    // nothing was left after the round before:
        if (blockIdx.x == 0 && threadIdx.x == 0) st->remaining[round % 3] = 0;        // nor is after this one
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->remaining[(round + 1) % 3] = 0;                       // the next round's count (last read a round ago)
        st->rounds = round + 1;
    }
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    int left = 0;
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const int v = static_cast<int>(row);
        if (state[v] != kUndecided) continue;
        const float dv = d[v];
        unsigned seen = 0u;
        const int end = rp[v + 1];
        for (int p = rp[v] + lane; p < end && !(seen & 1u); p += LANES) {
            const int u = ci[p];
            const float du = d[u];
            if (!amg_strong(v, u, va[p], theta2, dv, du)) continue;
            seen |= look(u, v, seed, state);
            const int uend = rp[u + 1];
            for (int q = rp[u]; q < uend; ++q) {
                const int w = ci[q];
                if (w == v || !amg_strong(u, w, va[q], theta2, du, d[w])) continue;
                seen |= look(w, v, seed, state);
            }
        }
        seen = group_or<LANES>(seen);
        if (seen & 1u) {
            if (lane == 0) state[v] = kOut;
        } else if (!(seen & 2u)) {
            if (lane == 0) state[v] = kRoot;
        } else {
            left += lane == 0;
        }
    }
    __shared__ int s_left[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) left += __shfl_xor(left, off, 64);
    if ((threadIdx.x & 63) == 0) s_left[threadIdx.x >> 6] = left;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBlock / 64; ++w) total += s_left[w];
        if (total > 0) atomicAdd(&st->remaining[round % 3], total);
    }
}

// rank[i] = 1 for a root (rank[n] = 0: the scan turns it into the number of roots)
__global__ __launch_bounds__(kBlock) void mis2_flags_kernel(int n, const int* __restrict__ state,
                                                            int* __restrict__ rank) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i <= n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        rank[i] = i < n && state[i] == kRoot ? 1 : 0;
    }
}

// first[v]: a root's own number; else that of the first root among v's strong neighbours in storage order; else -1
template <int LANES>
__global__ __launch_bounds__(kBlock)
void mis2_phase1_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const float* __restrict__ va,
                        const float* __restrict__ d, double theta2, const int* __restrict__ state,
                        const int* __restrict__ rank, int* __restrict__ first) {
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const int v = static_cast<int>(row);
        int result;
        if (state[v] == kRoot) {
            result = rank[v];
        } else {
            const float dv = d[v];
            int pos = INT_MAX;
            const int end = rp[v + 1];
            for (int p = rp[v] + lane; p < end; p += LANES) {
                const int u = ci[p];
                if (amg_strong(v, u, va[p], theta2, dv, d[u]) && state[u] == kRoot) {
                    pos = p;
                    break;
                }
            }
            pos = group_min<LANES>(pos);
            result = pos == INT_MAX ? -1 : rank[ci[pos]];
        }
        if (lane == 0) first[v] = result;
    }
}

// aggregate[v] = first[v], or for a vertex phase 1 left free the `first` of the column of its strong entry with the
// largest |v| among the columns phase 1 placed (the first in storage order on a tie), or -1; partial[b] = the smallest
// row workgroup b left at -1; st->count = the number of roots
template <int LANES>
__global__ __launch_bounds__(kBlock)
void mis2_phase2_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const float* __restrict__ va,
                        const float* __restrict__ d, double theta2, const int* __restrict__ first,
                        const int* __restrict__ rank, int* __restrict__ aggregate, int* __restrict__ partial,
                        Mis2State* __restrict__ st) {
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    int free_row = INT_MAX;
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const int v = static_cast<int>(row);
        int result = first[v];
        if (result == -1) {
            const float dv = d[v];
            float best_abs = -1.0f;
            int best_pos = INT_MAX;
            const int end = rp[v + 1];
            for (int p = rp[v] + lane; p < end; p += LANES) {
                const int u = ci[p];
                const float val = va[p];
                if (!amg_strong(v, u, val, theta2, dv, d[u]) || first[u] == -1) continue;
                const float a = fabsf(val);
                if (a > best_abs) {               // positions ascend: a tie keeps the earlier one
                    best_abs = a;
                    best_pos = p;
                }
            }
#pragma unroll
            for (int off = LANES / 2; off > 0; off >>= 1) {
                const float other_abs = __shfl_xor(best_abs, off, 64);
                const int other_pos = __shfl_xor(best_pos, off, 64);
                if (other_abs > best_abs || (other_abs == best_abs && other_pos < best_pos)) {
                    best_abs = other_abs;
                    best_pos = other_pos;
                }
            }
            if (best_pos != INT_MAX) result = first[ci[best_pos]];
        }
        if (lane == 0) {
            aggregate[v] = result;
            if (result == -1) free_row = min(free_row, v);
        }
    }
    free_row = block_min(free_row);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = free_row;
        if (blockIdx.x == 0) st->count = rank[n];
    }
}

// P's row pointers and values (its columns are the aggregate map)
__global__ __launch_bounds__(kBlock) void amg_prolongation_kernel(int n, int* __restrict__ p_rp,
                                                                  float* __restrict__ p_va) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i <= n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        p_rp[i] = static_cast<int>(i);
        if (i < n) p_va[i] = 1.0f;
    }
}

// s_i = float(-double(omega_p) / double(d_i)): the row scale of the smoothed prolongator
__global__ __launch_bounds__(kBlock) void amg_smoothing_scale_kernel(int n, float omega_p, const float* __restrict__ d,
                                                                     float* __restrict__ scale) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        scale[i] = static_cast<float>(-static_cast<double>(omega_p) / static_cast<double>(d[i]));
    }
}

int mis_lanes_for(const CSRMatrix& M) {
    if (int f = forced_lanes("mis_lanes")) return f;
    return pick_lanes_per_row(static_cast<float>(M.nnz) / static_cast<float>(std::max(M.num_rows, 1)));
}

// the device memory of the setup of levels of up to `rows` rows (aggregation = false: of their diagonals alone), and
// the mirror of its state
struct Scratch {
    solver::Workspace<Mis2State> ws;
    DevBuf<float> d;
    DevBuf<int> state, rank, first, partial, sums;    // partial: one slot per workgroup of the largest grid

    bool allocate(int rows, bool aggregation = true) {
        const long long scan_sums = device_scan_sums(device_scan_levels(static_cast<long long>(rows) + 1));
        bool ok = ws.allocate(0, 0) && dev_alloc(&d, rows) == hipSuccess &&
                  dev_alloc(&partial, dev::kMaxResidentBlocks) == hipSuccess;
        if (ok && aggregation) {
            ok = dev_alloc(&state, rows) == hipSuccess && dev_alloc(&rank, static_cast<long long>(rows) + 1) == hipSuccess &&
                 dev_alloc(&first, rows) == hipSuccess && dev_alloc(&sums, scan_sums) == hipSuccess;
        }
        if (!ok) (void)hipGetLastError();
        return ok;
    }
};

// d (and wd, with the check, when it is given) of M, and the smallest bad row into the state; not waited for
bool enqueue_diagonal(const CSRMatrix& M, float omega, float* d, float* wd, Scratch& sc, hipStream_t s) {
    const int n = M.num_rows;
    const int blocks = vec_grid(n);
    amg_diag_kernel<<<blocks, kBlock, 0, s>>>(n, M.d_row_ptrs, M.d_col_indices, M.d_values, omega, d, wd,
                                              sc.partial.get());
    min_fold_kernel<<<1, kBlock, 0, s>>>(sc.partial.get(), blocks, &sc.ws.state->bad_row);
    return hipGetLastError() == hipSuccess;
}

// The aggregation of M (n >= 1, structure valid, sc.d holds its diagonals) into d_aggregate; returns after the state
// (count, free_row, rounds; bad_row as enqueue_diagonal left it) has arrived in sc.ws.pinned[0].
bool aggregate_level(const CSRMatrix& M, float theta, unsigned seed, int* d_aggregate, Scratch& sc, hipStream_t s) {
    const int n = M.num_rows;
    const int lanes = mis_lanes_for(M);
    const int grid = capped_grid(n, kBlock / lanes);
    const double theta2 = static_cast<double>(theta) * static_cast<double>(theta);
    const int* rp = M.d_row_ptrs;
    const int* ci = M.d_col_indices;
    const float* va = M.d_values;
    solver::Workspace<Mis2State>& ws = sc.ws;
    mis2_init_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, sc.state.get(), ws.state);
    bool ok = hipGetLastError() == hipSuccess;
    ok = ok && solver::run_rounds(n, ws, s, [&](int round) {
        return with_lanes(lanes, [&](auto L) {
            mis2_round_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(n, rp, ci, va, sc.d.get(), theta2, seed,
                                                                          sc.state.get(), ws.state, round);
            return hipGetLastError();
        });
    });
    if (ok) {
        mis2_flags_kernel<<<vec_grid(static_cast<long long>(n) + 1), kBlock, 0, s>>>(n, sc.state.get(), sc.rank.get());
        ok = hipGetLastError() == hipSuccess &&
             device_exclusive_scan(sc.rank.get(), device_scan_levels(static_cast<long long>(n) + 1), sc.sums.get(), s) ==
                 hipSuccess;
    }
    if (ok) {
        ok = with_lanes(lanes, [&](auto L) {
            constexpr int kLanes = decltype(L)::value;
            mis2_phase1_kernel<kLanes><<<grid, kBlock, 0, s>>>(n, rp, ci, va, sc.d.get(), theta2, sc.state.get(),
                                                               sc.rank.get(), sc.first.get());
            mis2_phase2_kernel<kLanes><<<grid, kBlock, 0, s>>>(n, rp, ci, va, sc.d.get(), theta2, sc.first.get(),
                                                               sc.rank.get(), d_aggregate, sc.partial.get(), ws.state);
            return hipGetLastError();
        }) == hipSuccess;
        min_fold_kernel<<<1, kBlock, 0, s>>>(sc.partial.get(), grid, &ws.state->free_row);
        ok = ok && hipGetLastError() == hipSuccess;
    }
    return ws.read_back(ok, s);
}

// not device_arrays_strict: nnz < 0 fails here (there it counts as no entries), num_rows is the caller's to check
bool device_arrays_nnz_checked(const CSRMatrix* M) {
    return M->nnz >= 0 && M->d_row_ptrs && (M->nnz == 0 || (M->d_col_indices && M->d_values));
}

CSRMatrix device_view(const CSRMatrix* M) {
    CSRMatrix v{};
    v.num_rows = M->num_rows;
    v.num_cols = M->num_cols;
    v.nnz = M->nnz;
    v.d_row_ptrs = M->d_row_ptrs;
    v.d_col_indices = M->d_col_indices;
    v.d_values = M->d_values;
    return v;
}

float ms_since(std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - start).count();
}

struct DeviceBuilder {
    AMGHierarchy& H;
    AMGResult& res;
    Scratch& sc;
    hipStream_t stream;

    int fail(SpMVError e, int level = -1, int row = -1) {
        (void)hipGetLastError();
        res.error_code = code(e);
        res.bad_level = level;
        res.bad_row = row;
        return res.error_code;
    }

    // d into the scratch and wd = omega / d into the level (d_wd allocated by the first call); not waited for
    int diagonal_of(int l) {
        AMGLevel& lv = H.levels[static_cast<size_t>(l)];
        const size_t n = static_cast<size_t>(lv.view.num_rows);
        if (!lv.d_wd && hipMalloc(reinterpret_cast<void**>(&lv.d_wd), n * sizeof(float)) != hipSuccess) {
            return fail(SpMVError::CUDA_MALLOC);
        }
        if (!enqueue_diagonal(lv.view, H.config.jacobi_weight, sc.d.get(), lv.d_wd, sc, stream)) {
            return fail(SpMVError::KERNEL_LAUNCH);
        }
        return 0;
    }

    // the state read back on its own (a level that is not aggregated)
    int diagonal_checked(int l) {
        if (!sc.ws.read_back(true, stream, sizeof(Mis2State))) return fail(SpMVError::KERNEL_LAUNCH);
        return bad_diagonal(l);
    }

    int bad_diagonal(int l) {
        const int bad = sc.ws.pinned[0].bad_row;
        return bad != INT_MAX ? fail(SpMVError::INVALID_ARGUMENT, l, bad) : 0;
    }

    // P in device memory around the aggregate map, then P^T, A P and A_{l+1}; appends level l + 1
    int coarsen(int l, DevBuf<int>& map, int count) {
        const int n = H.levels[static_cast<size_t>(l)].view.num_rows;
        DevBuf<int> p_rp;
        DevBuf<float> p_va;
        if (dev_alloc(&p_rp, static_cast<long long>(n) + 1) != hipSuccess || dev_alloc(&p_va, n) != hipSuccess) {
            return fail(SpMVError::CUDA_MALLOC);
        }
        amg_prolongation_kernel<<<vec_grid(static_cast<long long>(n) + 1), kBlock, 0, stream>>>(n, p_rp.get(),
                                                                                                p_va.get());
        if (hipGetLastError() != hipSuccess) return fail(SpMVError::KERNEL_LAUNCH);
        CSRMatrix* P = new CSRMatrix{};       // device arrays only, owned: csr_destroy frees them
        P->num_rows = n;
        P->num_cols = count;
        P->nnz = n;
        P->d_row_ptrs = p_rp.release();
        P->d_col_indices = map.release();
        P->d_values = p_va.release();
        P->owns_device_memory = true;
        CSRMatrix* PT = csr_create(0, 0, 0);
        CSRMatrix* AP = csr_create(0, 0, 0);
        CSRMatrix* next = csr_create(0, 0, 0);
        CSRMatrix* AT = H.smoothed ? csr_create(0, 0, 0) : nullptr;
        CSRMatrix* smoothed_P = H.smoothed ? csr_create(0, 0, 0) : nullptr;
        {
            AMGLevel& lv = H.levels[static_cast<size_t>(l)];     // owners first: every exit frees them with H
            lv.P = P;
            lv.PT = PT;
            lv.AP = AP;
            lv.num_aggregates = count;
            if (H.smoothed) {                                    // the unit P made above is the tentative one
                lv.T = P;
                lv.P = smoothed_P;
                lv.AT = AT;
            }
        }
        H.levels.emplace_back();
        H.levels.back().A = next;
        if (!PT || !AP || !next || (H.smoothed && (!AT || !smoothed_P))) return fail(SpMVError::OUT_OF_MEMORY);
        if (H.smoothed) {
            if (const int status = amg_smooth_coarsen(H, l, sc.d.get(), false, stream)) {
                return fail(static_cast<SpMVError>(status));
            }
            H.levels.back().view = device_view(next);
            return 0;
        }
        int status = csr_transpose_gpu(PT, P);
        if (status == 0) status = spgemm_csr(AP, &H.levels[static_cast<size_t>(l)].view, P);
        if (status == 0) status = spgemm_csr(next, PT, AP);
        if (status != 0) return fail(static_cast<SpMVError>(status));
        H.levels.back().view = device_view(next);
        return 0;
    }
};

} // namespace

int amg_smooth_coarsen(AMGHierarchy& H, int l, const float* d_diag, bool refill, hipStream_t s) {
    AMGLevel& lv = H.levels[static_cast<size_t>(l)];
    CSRMatrix* next = H.levels[static_cast<size_t>(l) + 1].A;
    const int n = lv.view.num_rows;
    int status = refill ? spgemm_csr_numeric(lv.AT, &lv.view, lv.T) : spgemm_csr(lv.AT, &lv.view, lv.T);
    if (status != 0) return status;
    if (!refill) {
        const size_t floats = static_cast<size_t>(n) + static_cast<size_t>(lv.AT->nnz);
        if (hipMalloc(reinterpret_cast<void**>(&lv.d_s), floats * sizeof(float)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&lv.d_res), static_cast<size_t>(n) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return code(SpMVError::CUDA_MALLOC);
        }
    }
    amg_smoothing_scale_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, H.smoothing.prolongator_weight, d_diag, lv.d_s);
    if (hipGetLastError() != hipSuccess) return code(SpMVError::KERNEL_LAUNCH);
    CSRMatrix S = device_view(lv.AT);                      // AT's structure around its own values
    S.d_values = lv.d_s + n;
    status = csr_scale_gpu(lv.AT, lv.d_s, nullptr, S.d_values);
    if (status == 0) status = refill ? csr_add_numeric(lv.P, 1.0f, lv.T, 1.0f, &S) : csr_add(lv.P, 1.0f, lv.T, 1.0f, &S);
    if (status == 0) status = csr_transpose_gpu(lv.PT, lv.P);
    if (status == 0) status = refill ? spgemm_csr_numeric(lv.AP, &lv.view, lv.P) : spgemm_csr(lv.AP, &lv.view, lv.P);
    if (status == 0) status = refill ? spgemm_csr_numeric(next, lv.PT, lv.AP) : spgemm_csr(next, lv.PT, lv.AP);
    if (status != 0) return status;
    lv.p_lanes = pick_lanes_per_row(static_cast<float>(lv.P->nnz) / static_cast<float>(std::max(lv.P->num_rows, 1)));
    lv.pt_lanes = pick_lanes_per_row(static_cast<float>(lv.PT->nnz) / static_cast<float>(std::max(lv.PT->num_rows, 1)));
    return 0;
}

AMGResult amg_update_device(AMGHierarchy* H, const CSRMatrix* A) {
    const auto start = std::chrono::steady_clock::now();
    AMGResult res;
    const TraceRange range("spmv:amg_update");
    hipStream_t stream = current_stream();
    Scratch sc;
    DeviceBuilder b{*H, res, sc, stream};
    if (!sc.allocate(H->num_rows, false)) {
        b.fail(SpMVError::CUDA_MALLOC);
        return res;
    }
    H->levels[0].view = device_view(A);
    if (const int status = structure_checked(A, stream)) {
        b.fail(static_cast<SpMVError>(status));
        return res;
    }
    const int levels = static_cast<int>(H->levels.size());
    for (int l = 0; l < levels; ++l) {
        if (b.diagonal_of(l) != 0 || b.diagonal_checked(l) != 0) return res;
        if (l + 1 == levels) break;
        AMGLevel& lv = H->levels[static_cast<size_t>(l)];
        int status = 0;
        if (H->smoothed) {
            status = amg_smooth_coarsen(*H, l, sc.d.get(), true, stream);
        } else {
            status = spgemm_csr_numeric(lv.AP, &lv.view, lv.P);
            if (status == 0) status = spgemm_csr_numeric(H->levels[static_cast<size_t>(l) + 1].A, lv.PT, lv.AP);
        }
        if (status != 0) {
            b.fail(static_cast<SpMVError>(status));
            return res;
        }
    }
    if (amg_finish(*H, res, stream) != 0) return res;
    res.setup_ms = ms_since(start);
    return res;
}

} // namespace detail

int amg_aggregate_mis2_gpu(const CSRMatrix* A, float strength, unsigned seed, int* d_aggregate, int* num_aggregates,
                           int* rounds) {
    using namespace detail;
    if (!A || !d_aggregate || !num_aggregates) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows < 0 || !device_arrays_nnz_checked(A)) return code(SpMVError::INVALID_FORMAT);
    if (!(strength >= 0.0f)) return code(SpMVError::INVALID_ARGUMENT);
    hipStream_t stream = current_stream();
    if (const int status = structure_checked(A, stream)) return status;
    if (A->num_rows == 0) {
        *num_aggregates = 0;
        if (rounds) *rounds = 0;
        return 0;
    }
    const TraceRange range("spmv:amg_aggregate_mis2_gpu");
    Scratch sc;
    if (!sc.allocate(A->num_rows)) return code(SpMVError::CUDA_MALLOC);
    const CSRMatrix view = device_view(A);
    if (!enqueue_diagonal(view, 1.0f, sc.d.get(), nullptr, sc, stream) ||
        !aggregate_level(view, strength, seed, d_aggregate, sc, stream)) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    *num_aggregates = sc.ws.pinned[0].count;
    if (rounds) *rounds = sc.ws.pinned[0].rounds;
    return 0;
}

namespace detail {
namespace {

// amg_setup_device (smoothing == nullptr) and amg_setup_smoothed_device
AMGResult setup_device(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config, const AMGSmoothing* smoothing,
                       unsigned seed) {
    const auto start = std::chrono::steady_clock::now();
    AMGResult res;
    const auto fail = [&res](SpMVError e) {
        res.error_code = code(e);
        return res;
    };
    if (out) *out = nullptr;
    if (!out || !A) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols || A->num_rows < 1) return fail(SpMVError::INVALID_DIMENSION);
    if (!device_arrays_nnz_checked(A)) return fail(SpMVError::INVALID_FORMAT);
    const AMGConfig defaults;
    const AMGConfig& cfg = config ? *config : defaults;
    if (!amg_config_ok(cfg)) return fail(SpMVError::INVALID_ARGUMENT);
    if (smoothing && !amg_smoothing_ok(*smoothing)) return fail(SpMVError::INVALID_ARGUMENT);

    const TraceRange range(smoothing ? "spmv:amg_setup_smoothed_device" : "spmv:amg_setup_device");
    hipStream_t stream = current_stream();
    std::unique_ptr<AMGHierarchy, void (*)(AMGHierarchy*)> H(new AMGHierarchy, amg_destroy);
    H->config = cfg;
    H->num_rows = A->num_rows;
    H->nnz = A->nnz;
    H->device_built = true;
    if (smoothing) {
        H->smoothed = true;
        H->smoothing = *smoothing;
    }
    float theta = cfg.strength;      // theta_l: constant on a plain hierarchy
    H->levels.emplace_back();
    H->levels[0].view = device_view(A);
    Scratch sc;
    DeviceBuilder b{*H, res, sc, stream};
    if (!sc.allocate(A->num_rows)) return fail(SpMVError::CUDA_MALLOC);
    if (const int status = structure_checked(A, stream)) return fail(static_cast<SpMVError>(status));
    for (int l = 0;; ++l) {
        if (b.diagonal_of(l) != 0) return res;
        const CSRMatrix view = H->levels[static_cast<size_t>(l)].view;
        const int n = view.num_rows;
        if (n <= cfg.coarse_rows || l + 1 == cfg.max_levels) {
            if (b.diagonal_checked(l) != 0 || amg_level_workspace(*H, res, l) != 0) return res;
            break;
        }
        DevBuf<int> map;
        if (dev_alloc(&map, n) != hipSuccess) {
            b.fail(SpMVError::CUDA_MALLOC);
            return res;
        }
        if (!aggregate_level(view, theta, seed, map.get(), sc, stream)) {
            b.fail(SpMVError::KERNEL_LAUNCH);
            return res;
        }
        if (b.bad_diagonal(l) != 0 || amg_level_workspace(*H, res, l) != 0) return res;
        const Mis2State& st = sc.ws.pinned[0];
        if (st.free_row != INT_MAX) {
            b.fail(SpMVError::INVALID_ARGUMENT, l, st.free_row);
            return res;
        }
        const int count = st.count;
        if (count == n) break;                          // nothing is strong any more
        H->levels[static_cast<size_t>(l)].rounds = st.rounds;
        if (b.coarsen(l, map, count) != 0) return res;
        if (smoothing) theta = theta * smoothing->strength_decay;
    }
    if (amg_finish(*H, res, stream) != 0) return res;
    res.setup_ms = ms_since(start);
    *out = H.release();
    return res;
}

} // namespace
} // namespace detail

AMGResult amg_setup_device(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config, unsigned seed) {
    return detail::setup_device(out, A, config, nullptr, seed);
}

AMGResult amg_setup_smoothed_device(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config,
                                    const AMGSmoothing* smoothing, unsigned seed) {
    const AMGSmoothing defaults;
    return detail::setup_device(out, A, config, smoothing ? smoothing : &defaults, seed);
}

} // namespace spmv
