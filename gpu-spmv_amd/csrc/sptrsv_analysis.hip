// sptrsv_analysis.hip — the level analysis of sptrsv_csr on the device (include/spmv/sptrsv.h sptrsv_analyze_device,
// DESIGN.md §4.23): what schedule_for() of sptrsv_host.cpp computes on the host, from the device arrays alone.
//
//   statistics   one pass over A, 1-64 lanes per row: dep[i] = stored off-diagonal entries of row i inside the
//                triangle (duplicates counted), the lowest row without a diagonal, the lowest row whose columns are
//                not strictly ascending, the triangle's entry count; rows with dep == 0 are level 0 and open the queue.
//   transpose    transpose_build: row c of A^T lists the rows that store an entry in column c, once per stored entry.
//   one-sided    LOWER schedules of sorted matrices with every diagonal: row i of A against row i of A^T.
//   peeling      round r walks the queue slice of level r; for every dependent inside the triangle it decrements
//                dep[]; the decrement that reaches zero sets level = r + 1 and appends the row.  Every stored entry
//                inside the triangle is visited once.  A frontier wider than kSptrsvNarrowRows is one launch over
//                the chip; runs of narrower ones are walked by ONE workgroup with a barrier in between, at most
//                kSptrsvMaxRunLevels of them per launch (the solve's own launch rule).
//   sort         the stable sort of the rows by level is the transpose of the n x num_levels matrix with the entry
//                (i, level[i]) in row i (reorder.hip's trick): its row pointers are level_ptr, its columns the order.
//
// The atomics are integer and their outcome does not depend on arrival order: dep[] is a counter whose zero crossing
// happens exactly once whoever causes it, level = r + 1 is the same from every writer of round r, the queue tail
// decides only WHERE inside its level's slice a row lies, and the slice is a set: the sort, not the queue, orders
// the rows.  The statistics are min / sum reductions.  No workgroup waits for another; order is stream order.
#include "solver_common.h"

#include <climits>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using dev::capped_grid;
using dev::find_column;
using dev::kBlock;
using dev::vec_grid;
using dev::with_lanes;

constexpr int kHubDependents = 2048;    // a column with more dependents than this is walked by a whole wavefront

// The device state of one analysis.  Round r reads level r's rows from queue[start[(r + 2) % 3] ..] (remaining[(r + 2)
// % 3] of them), appends level r + 1 at start[r % 3] + remaining[r % 3]++ and zeroes remaining[(r + 1) % 3], last
// read a round ago (csr_color's rotation).
struct PeelState {
    int remaining[3];
    int start[3];
    int round;              // the round the next single-workgroup launch begins with
    int wide_round;         // the last round a wide launch walked, -1 before the first
    int done;               // round `levels` found an empty frontier
    int levels;
    int first_missing;      // INT_MAX = none, as the two below
    int first_unsorted;
    int one_sided;
    int reserved;
    unsigned long long triangle_nnz;
};

// The counters other workgroups (or other wavefronts of this one) update with atomics are read and written past
// the first-level cache.
__device__ __forceinline__ int peek(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void poke(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0u)));
}

template <int LANES>
__device__ __forceinline__ int group_add(int v) {
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Appends `row` for every lane with `hit` at base + (*tail)++: one atomic per wavefront.  Called by whole wavefronts.
// Every row joins the queue once, so a position is always below n; the comparison only makes sure that a broken
// invariant would show as a wrong schedule and never as a store outside the queue.
__device__ __forceinline__ void append_rows(bool hit, int row, int base, int* tail, int* queue, int n) {
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) return;
    const int leader = __builtin_ctzll(m);
    int first = 0;
    if (static_cast<int>(threadIdx.x & 63) == leader) first = atomicAdd(tail, __popcll(m));
    first = __shfl(first, leader, 64);
    const int at = base + first + lanes_below(m);
    if (hit && at >= 0 && at < n) queue[at] = row;
}

__global__ void analysis_init_kernel(PeelState* state) {
    state->remaining[0] = state->remaining[1] = state->remaining[2] = 0;
    state->start[0] = state->start[1] = state->start[2] = 0;
    state->round = 0;
    state->wide_round = -1;
    state->done = 0;
    state->levels = 0;
    state->first_missing = INT_MAX;
    state->first_unsorted = INT_MAX;
    state->one_sided = INT_MAX;
    state->reserved = 0;
    state->triangle_nnz = 0ull;
}

// ---- statistics: one pass over A (validated), LANES lanes per row ----
template <int LANES>
__global__ __launch_bounds__(kBlock)
void analysis_stats_kernel(int n, int upper, const int* __restrict__ rp, const int* __restrict__ ci,
                           int* __restrict__ dep, int* __restrict__ level, int* __restrict__ queue,
                           PeelState* state) {
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int in_wave = (threadIdx.x & 63) / LANES;
    int missing = INT_MAX, unsorted = INT_MAX;
    long long inside = 0;
    // every lane of a wavefront makes every trip (the appends are wavefront-wide)
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row - in_wave < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const bool have = row < n;
        const int i = static_cast<int>(row);
        int count = 0, triangle = 0, diagonal = 0, disorder = 0;
        if (have) {
            const int begin = rp[i], end = rp[i + 1];
            for (int j = begin + lane; j < end; j += LANES) {
                const int c = ci[j];
                if (c == i) {
                    diagonal = 1;
                    ++triangle;
                } else if (upper ? c > i : c < i) {
                    ++count;
                    ++triangle;
                }
                if (j > begin && c <= ci[j - 1]) disorder = 1;
            }
        }
        count = group_add<LANES>(count);
        triangle = group_add<LANES>(triangle);
        diagonal = group_add<LANES>(diagonal);
        disorder = group_add<LANES>(disorder);
        const bool mine = have && lane == 0;
        if (mine) {
            dep[i] = count;
            if (count == 0) level[i] = 0;
            if (!diagonal) missing = min(missing, i);
            if (disorder) unsorted = min(unsorted, i);
            inside += triangle;
        }
        append_rows(mine && count == 0, i, 0, &state->remaining[2], queue, n);
    }
    for (int off = 32; off > 0; off >>= 1) {
        missing = min(missing, __shfl_xor(missing, off, 64));
        unsorted = min(unsorted, __shfl_xor(unsorted, off, 64));
        inside += __shfl_xor(inside, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (missing != INT_MAX) atomicMin(&state->first_missing, missing);
        if (unsorted != INT_MAX) atomicMin(&state->first_unsorted, unsorted);
        if (inside != 0) atomicAdd(&state->triangle_nnz, static_cast<unsigned long long>(inside));
    }
}

// ---- one_sided_row: the lowest row i that stores an (i, k), k != i, whose (k, i) is not stored.  Rows strictly
// ascending and every diagonal stored (else the kernel leaves at once): row i of A^T lists the k with a stored
// (k, i) in ascending order, so a symmetric pattern matches position by position and only a mismatch searches. ----
template <int LANES>
__global__ __launch_bounds__(kBlock)
void analysis_one_sided_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                               const int* __restrict__ trp, const int* __restrict__ tci, PeelState* state) {
    if (state->first_missing != INT_MAX || state->first_unsorted != INT_MAX) return;
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    int lowest = INT_MAX;
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const int i = static_cast<int>(row);
        const int begin = rp[i], len = rp[i + 1] - begin;
        const int tbegin = trp[i], tlen = trp[i + 1] - tbegin;
        for (int e = lane; e < len; e += LANES) {
            const int k = ci[begin + e];
            if (k == i) continue;
            if (e < tlen && tci[tbegin + e] == k) continue;
            if (find_column(tci, tbegin, tbegin + tlen, k) < 0) lowest = min(lowest, i);
        }
    }
    for (int off = 32; off > 0; off >>= 1) lowest = min(lowest, __shfl_xor(lowest, off, 64));
    if ((threadIdx.x & 63) == 0 && lowest != INT_MAX) atomicMin(&state->one_sided, lowest);
}

// ---- peeling ----
// The dependents of column c at positions j, j + step, ... < end of A^T, by the lanes of a whole wavefront (each with
// its own c, j, end): every one inside the triangle loses a dependency, and the one that had a single one left is
// of level next_level and joins the queue at base + (*tail)++.
__device__ __forceinline__ void release_dependents(int c, int j, int end, int step, int upper,
                                                   const int* __restrict__ tci, int* dep, int* level, int* queue,
                                                   int base, int* tail, int next_level, int n) {
    for (;;) {
        const bool active = j < end;
        if (!__any(active)) break;
        bool hit = false;
        int d = 0;
        if (active) {
            d = tci[j];
            if (upper ? d < c : d > c) hit = atomicSub(&dep[d], 1) == 1;
        }
        if (hit) level[d] = next_level;
        append_rows(hit, d, base, tail, queue, n);
        j += step;
    }
}

// The queue slice [begin, begin + size) of one level, LANES lanes per row of it, strided over by the `groups` lane
// groups of the launch of which this thread's is number `group`.  Whole wavefronts.
template <int LANES>
__device__ __forceinline__ void peel_slice(long long group, long long groups, int begin, int size, int upper,
                                           const int* __restrict__ trp, const int* __restrict__ tci, int* dep,
                                           int* level, int* queue, int* tail, int next_level, int n) {
    const int lane = threadIdx.x % LANES;
    const int wave_lane = threadIdx.x & 63;
    const int in_wave = wave_lane / LANES;
    const int base = begin + size;
    for (long long q = group; q - in_wave < size; q += groups) {
        int c = -1, j = 0, end = 0;
        if (q < size && begin + q < n) c = peek(&queue[begin + q]);
        if (c >= 0 && c < n) {                                    // (every queued row: see append_rows)
            j = trp[c];
            end = trp[c + 1];
        }
        const bool hub = LANES < 64 && end - j > kHubDependents;
        if (hub) end = j;                                         // left to the whole wavefront, below
        release_dependents(c, j + lane, end, LANES, upper, tci, dep, level, queue, base, tail, next_level, n);
        unsigned long long hubs = __ballot(hub && lane == 0);
        while (hubs != 0ull) {
            const int owner = __builtin_ctzll(hubs);
            hubs &= hubs - 1ull;
            const int hc = __shfl(c, owner, 64);
            release_dependents(hc, trp[hc] + wave_lane, trp[hc + 1], 64, upper, tci, dep, level, queue, base, tail,
                               next_level, n);
        }
    }
}

// One wide round: the round the single-workgroup launch before it stopped at, when its frontier is wider than
// kSptrsvNarrowRows; nothing otherwise.  Thread 0 of workgroup 0 turns the rotation: nothing it writes is read
// by this launch.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void analysis_peel_wide_kernel(int n, int upper, const int* __restrict__ trp, const int* __restrict__ tci, int* dep,
                               int* level, int* queue, PeelState* state) {
    if (state->done) return;
    const int r = state->round;
    const int size = state->remaining[(r + 2) % 3];
    if (size <= kSptrsvNarrowRows) return;
    const int begin = state->start[(r + 2) % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        poke(&state->remaining[(r + 1) % 3], 0);                  // (next to a word other workgroups add to)
        poke(&state->start[r % 3], begin + size);
        poke(&state->wide_round, r);
    }
    constexpr int kRows = kBlock / LANES;
    peel_slice<LANES>(static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES,
                      static_cast<long long>(gridDim.x) * kRows, begin, size, upper, trp, tci, dep, level, queue,
                      &state->remaining[r % 3], r + 1, n);
}

// A run of narrow rounds by one workgroup: from state->round (one further when the wide launch has walked that one)
// until the frontier is empty (done), wider than kSptrsvNarrowRows (the wide launch's) or kSptrsvMaxRunLevels rounds
// were walked.  The barrier between two rounds orders the appends of one before the reads of the next.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void analysis_peel_run_kernel(int n, int upper, const int* __restrict__ trp, const int* __restrict__ tci, int* dep,
                              int* level, int* queue, PeelState* state) {
    if (state->done) return;
    int r = state->round;
    if (state->wide_round == r) ++r;
    constexpr int kRows = kBlock / LANES;
    for (int walked = 0;; ++walked) {
        const int size = peek(&state->remaining[(r + 2) % 3]);    // the same in every thread: complete since the barrier
        const int begin = peek(&state->start[(r + 2) % 3]);
        if (size == 0 || size > kSptrsvNarrowRows || walked == kSptrsvMaxRunLevels) {
            if (threadIdx.x == 0) {
                state->round = r;
                if (size == 0) {
                    state->levels = r;
                    state->done = 1;
                }
            }
            return;
        }
        if (threadIdx.x == 0) {
            poke(&state->remaining[(r + 1) % 3], 0);
            poke(&state->start[r % 3], begin + size);
        }
        peel_slice<LANES>(threadIdx.x / LANES, kRows, begin, size, upper, trp, tci, dep, level, queue,
                          &state->remaining[r % 3], r + 1, n);
        __syncthreads();
        ++r;
    }
}

// lanes per row for rows of `mean` entries walked one entry per lane and step
int lanes_for_mean(double mean) {
    int lanes = 1;
    while (lanes < 64 && lanes < mean) lanes <<= 1;
    return lanes;
}

} // namespace

int sptrsv_analysis_device(const CSRMatrix* A, int uplo, hipStream_t s, SptrsvSchedule* out,
                           std::vector<int>* level_ptr) {
    const int n = A->num_rows;
    const long long nnz = A->nnz;
    const int upper = uplo == SpTRSVConfig::UPPER ? 1 : 0;

    // the device pass over the structure, before any kernel follows a row pointer or a column
    const int checked = structure_checked(A, s);
    if (checked != 0) return checked;

    solver::Workspace<PeelState> ws;
    DevBuf<int> dep, level, queue;
    if (!ws.allocate(0, 0) || dev_alloc(&dep, n) != hipSuccess || dev_alloc(&level, n) != hipSuccess ||
        dev_alloc(&queue, static_cast<long long>(n) + 1) != hipSuccess) {
        return fail(SpMVError::CUDA_MALLOC);
    }
    PeelState* state = ws.state;

    analysis_init_kernel<<<1, 1, 0, s>>>(state);
    bool ok = hipGetLastError() == hipSuccess;
    const int forced = forced_lanes("analysis_lanes");            // tests reach every instantiation
    const int row_lanes = forced ? forced : pick_lanes_per_row(static_cast<float>(nnz) / static_cast<float>(n));
    ok = ok && with_lanes(row_lanes, [&](auto L) {
        constexpr int kLanes = decltype(L)::value;
        analysis_stats_kernel<kLanes><<<capped_grid(n, kBlock / kLanes), kBlock, 0, s>>>(
            n, upper, A->d_row_ptrs, A->d_col_indices, dep.get(), level.get(), queue.get(), state);
        return hipGetLastError();
    }) == hipSuccess;
    if (!ok) return fail(SpMVError::KERNEL_LAUNCH);

    DeviceCsrArrays at;
    const ReleaseOnExit release_at{&at};
    const int transposed = transpose_build(A, &at, s);            // (waits for the stream)
    if (transposed != 0) return transposed;

    if (!upper) {
        ok = with_lanes(row_lanes, [&](auto L) {
            constexpr int kLanes = decltype(L)::value;
            analysis_one_sided_kernel<kLanes><<<capped_grid(n, kBlock / kLanes), kBlock, 0, s>>>(
                n, A->d_row_ptrs, A->d_col_indices, at.row_ptrs, at.col_indices, state);
            return hipGetLastError();
        }) == hipSuccess;
    }
    if (!ws.read_back(ok, s)) return fail(SpMVError::KERNEL_LAUNCH);
    const long long triangle_nnz = static_cast<long long>(ws.pinned[0].triangle_nnz);

    // ---- the rounds: pairs of (run of narrow rounds, one wide round), in batches with a look at the state between.
    // A pair that does not find the end walks at least one round and there are at most n levels, so n + 1 pairs find
    // the end of any input. ----
    const int lanes = forced ? forced : lanes_for_mean(static_cast<double>(triangle_nnz) / n);
    const int wide_grid = capped_grid(n, kBlock / lanes);
    const long long limit = static_cast<long long>(n) + 1;
    long long enqueued = 0;
    bool done = false;
    for (long long batch = 0; ok && !done; ++batch) {
        const long long todo = std::min<long long>(solver::kRoundsPerBatch, limit - enqueued);
        for (long long t = 0; t < todo && ok; ++t, ++enqueued) {
            ok = with_lanes(lanes, [&](auto L) {
                constexpr int kLanes = decltype(L)::value;
                analysis_peel_run_kernel<kLanes><<<1, kBlock, 0, s>>>(n, upper, at.row_ptrs, at.col_indices,
                                                                      dep.get(), level.get(), queue.get(), state);
                analysis_peel_wide_kernel<kLanes><<<wide_grid, kBlock, 0, s>>>(n, upper, at.row_ptrs, at.col_indices,
                                                                               dep.get(), level.get(), queue.get(),
                                                                               state);
                return hipGetLastError();
            }) == hipSuccess;
        }
        ok = ok && ws.publish(batch, sizeof(PeelState), s);
        const bool last = enqueued >= limit;
        const long long look = last ? batch + 1 : batch;          // the last batch is waited for at once
        if (ok && look >= 1) {
            const PeelState* seen = ws.wait_previous(look);
            ok = seen != nullptr;
            if (ok) done = seen->done != 0;
            if (ok && last && !done) ok = false;                  // cannot happen: see above
        }
    }
    if (!ws.read_back(ok, s)) {                                   // (every launch has ended: the transpose may go)
        (void)hipStreamSynchronize(s);
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    const PeelState result = ws.pinned[0];
    at.release();
    if (!result.done || result.levels < 1 || result.levels > n) return fail(SpMVError::KERNEL_LAUNCH);

    // ---- rows by level: row l of the transpose of the n x levels matrix with (i, level[i]) lists level l's rows in
    // ascending order; the values are never looked at ----
    const long long count = static_cast<long long>(n) + 1;
    if (launch_iota(count, queue.get(), vec_grid(count), s) != hipSuccess) return fail(SpMVError::KERNEL_LAUNCH);
    CSRMatrix byrow{};
    byrow.num_rows = n;
    byrow.num_cols = result.levels;
    byrow.nnz = n;
    byrow.d_row_ptrs = queue.get();
    byrow.d_col_indices = level.get();
    byrow.d_values = reinterpret_cast<float*>(level.get());
    DeviceCsrArrays bylevel;
    const int sorted = transpose_build(&byrow, &bylevel, s);
    if (sorted != 0) return sorted == code(SpMVError::INVALID_FORMAT) ? fail(SpMVError::KERNEL_LAUNCH) : sorted;
    level_ptr->assign(static_cast<size_t>(result.levels) + 1, 0);
    if (hipMemcpyAsync(level_ptr->data(), bylevel.row_ptrs, level_ptr->size() * sizeof(int), hipMemcpyDeviceToHost,
                       s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        bylevel.release();
        return fail(SpMVError::CUDA_MEMCPY);
    }
    (void)hipFree(bylevel.values);
    out->d_level_ptr = bylevel.row_ptrs;                          // the schedule owns them now
    out->d_order = bylevel.col_indices;
    out->num_levels = result.levels;
    out->triangle_nnz = static_cast<long long>(result.triangle_nnz);
    out->first_missing_diagonal = result.first_missing == INT_MAX ? -1 : result.first_missing;
    out->first_unsorted_row = result.first_unsorted == INT_MAX ? -1 : result.first_unsorted;
    out->one_sided_row = result.one_sided == INT_MAX ? -1 : result.one_sided;
    out->built_on_device = true;
    return code(SpMVError::SUCCESS);
}

} // namespace detail
} // namespace spmv
