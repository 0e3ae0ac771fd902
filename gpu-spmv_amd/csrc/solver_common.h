// solver_common.h — what the device-resident iterative solvers (cg.hip, cg_multi.hip, bicgstab.hip, gmres.hip,
// eigs.hip) share.
// Device side: the deterministic fp64 dot-product partials and their fixed-order fold, and diag_kernel, the one
// setup kernel that sums every row's diagonal.  Host side: the argument predicates (device_arrays, ranges_overlap),
// and the parts every solve() is built from:
//   Workspace<State>   the device memory of one solve, the two-deep pinned mirror of its state (publish /
//                      wait_previous) and the blocking read-backs (read_back, finish_timed)
//   run_rounds         the host loop of the algorithms in rounds (csr_color, MIS-2), built on that mirror
//   TriangularPair     M given as two triangles in one CSR matrix (IC, ILU): both schedules, then apply()
//   TiledEngine        the LDS-tiled engine's part in one solve: when the plan is built, and when it is dropped
// Each solver keeps its own loop and its own order of checks; nothing here calls back into one.  The launch layer
// (grid sizes, with_lanes) is device_common.h's, for every kernel file.  Internal: not installed under include/.
#ifndef SPMV_AMD_SOLVER_COMMON_H
#define SPMV_AMD_SOLVER_COMMON_H

#include "device_common.h"
#include "internal.h"
#include "tiled.h"
#include "spmv/sptrsv.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <type_traits>

namespace spmv {
namespace detail {
namespace solver {

using dev::kBlock;
using dev::kMaxResidentBlocks;
using dev::capped_grid;
using dev::vec_grid;
using dev::with_lanes;

// Sums part[i * stride] (and part[i * stride + 1] when stride > 1 and `pair`) over i < count in a fixed order,
// broadcast to every thread: each thread folds a fixed strided subset, then block_sum2's fixed butterfly and wave
// order.  pair = false reads nothing but part[i * stride] (b comes back 0): for a single value per group whose
// neighbour may lie past the end of the array.
__device__ __forceinline__ void fold_partials(const double* __restrict__ part, int count, int stride,
                                              double& a, double& b, bool pair = true) {
    __shared__ double s_fold[2];
    a = 0.0;
    b = 0.0;
    for (int i = threadIdx.x; i < count; i += kBlock) {
        a += part[static_cast<long long>(i) * stride];
        if (stride > 1 && pair) b += part[static_cast<long long>(i) * stride + 1];
    }
    dev::block_sum2(a, b);
    if (threadIdx.x == 0) {
        s_fold[0] = a;
        s_fold[1] = b;
    }
    __syncthreads();
    a = s_fold[0];
    b = s_fold[1];
}

__device__ __forceinline__ double prod64(float a, float b) {
    return static_cast<double>(a) * static_cast<double>(b);   // exact: 24 + 24 bits fit in fp64
}

// Which sums of a row's stored (i,i) entries diag_kernel accepts: CG's Jacobi (> 0), an IC factor (> 0 and finite),
// BiCGSTAB's and GMRES's Jacobi and an LU factor (any sign, not 0, finite).  A row without a stored diagonal fails all.
enum class DiagRule { POSITIVE, POSITIVE_FINITE, NONZERO_FINITE };

// d = the sum of row i's stored (i,i) entries (fp32, storage order); dinv[i] = 1 / d, or 0 for a row RULE rejects
// (dinv == nullptr: the check alone); *bad_flag = 1 if any row is rejected (every writer stores the same 1).  One
// thread per row: setup only.
template <DiagRule RULE>
__global__ __launch_bounds__(kBlock)
void diag_kernel(int n, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                 const float* __restrict__ vals, float* __restrict__ dinv, int* __restrict__ bad_flag) {
    int bad = 0;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float d = 0.0f;
        int found = 0;
        for (int j = row_ptrs[i]; j < row_ptrs[i + 1]; ++j) {
            if (cols[j] == i) {
                d = __fadd_rn(d, vals[j]);
                found = 1;
            }
        }
        bool ok = found;
        if constexpr (RULE == DiagRule::NONZERO_FINITE) ok = ok && d != 0.0f && isfinite(d);
        else if constexpr (RULE == DiagRule::POSITIVE_FINITE) ok = ok && d > 0.0f && isfinite(d);
        else ok = ok && d > 0.0f;
        if (dinv) dinv[i] = ok ? __fdiv_rn(1.0f, d) : 0.0f;
        bad |= !ok;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *bad_flag = 1;
}

inline bool ranges_overlap(const float* a, const float* b, long long n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = static_cast<uintptr_t>(n) * sizeof(float);
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

// the solvers' name for the strict rule of internal.h
inline bool device_arrays(const CSRMatrix* M) { return device_arrays_strict(M); }

template <DiagRule RULE>
hipError_t launch_diag(const CSRMatrix* M, float* dinv, int* bad_flag, hipStream_t s) {
    diag_kernel<RULE><<<vec_grid(M->num_rows), kBlock, 0, s>>>(M->num_rows, M->d_row_ptrs, M->d_col_indices,
                                                               M->d_values, dinv, bad_flag);
    return hipGetLastError();
}

// ||b|| == 0: x = 0, waited for.  false (and the HIP error cleared) when that fails.
inline bool zero_solution(float* d_x, size_t n, hipStream_t s) {
    const bool ok = hipMemsetAsync(d_x, 0, n * sizeof(float), s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok;
}

// M^-1 for an M stored as its two triangles in one CSR matrix: out = U^-1 (L^-1 in).  unit_lower: L's diagonal is an
// implied 1 (ILU: 1) or the stored one (IC, where U = L^T: 0); U's is always the stored one.
struct TriangularPair {
    const CSRMatrix* M = nullptr;
    std::shared_ptr<const SptrsvSchedule> lower, upper;
    int lower_lanes = 1, upper_lanes = 1;
    int unit_lower = 0;

    // Both schedules of M, which validate its structure before any kernel walks it.  Ahead of the timed loop: a
    // build synchronises the stream.  Returns 0 or the SpMVError code of the schedule that failed.
    int build(const CSRMatrix* matrix, int unit_lower_diagonal, hipStream_t s) {
        M = matrix;
        unit_lower = unit_lower_diagonal;
        float analysis_ms = 0.0f;
        int status = sptrsv_schedule_for(M, SpTRSVConfig::LOWER, s, &lower, &analysis_ms);
        if (status == 0) status = sptrsv_schedule_for(M, SpTRSVConfig::UPPER, s, &upper, &analysis_ms);
        if (status != 0) return status;
        lower_lanes = sptrsv_lanes_for(*lower);
        upper_lanes = sptrsv_lanes_for(*upper);
        return 0;
    }
    // LOWER into out, then UPPER in place
    bool apply(const float* in, float* out, hipStream_t s) const {
        return launch_sptrsv(*lower, M, in, out, SpTRSVConfig::LOWER, unit_lower, false, lower_lanes, s) ==
                   hipSuccess &&
               launch_sptrsv(*upper, M, out, out, SpTRSVConfig::UPPER, 0, false, upper_lanes, s) == hipSuccess;
    }
    // the k-wide form: one launch sequence per triangle whatever k
    bool apply(const SptrsvMultiArrays& down, const SptrsvMultiArrays& up, hipStream_t s) const {
        return launch_sptrsv_multi(*lower, M, down, SpTRSVConfig::LOWER, unit_lower, false, lower_lanes, s) ==
                   hipSuccess &&
               launch_sptrsv_multi(*upper, M, up, SpTRSVConfig::UPPER, 0, false, upper_lanes, s) == hipSuccess;
    }
};

// Device memory of one solve, freed on every exit.  State is the solver's device state.
template <class State>
struct Workspace {
    float* vec = nullptr;          // the solver's n-float vectors
    double* part = nullptr;        // partial sums
    State* state = nullptr;
    State* pinned = nullptr;       // [2] pinned host mirror
    hipEvent_t seen[2] = {nullptr, nullptr};

    // false (and the HIP error cleared) when any allocation fails
    bool allocate(size_t vec_floats, size_t part_doubles) {
        const bool ok = hipMalloc(reinterpret_cast<void**>(&vec), vec_floats * sizeof(float)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&part), part_doubles * sizeof(double)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void**>(&state), sizeof(State)) == hipSuccess &&
                        hipHostMalloc(reinterpret_cast<void**>(&pinned), 2 * sizeof(State)) == hipSuccess &&
                        hipEventCreateWithFlags(&seen[0], hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&seen[1], hipEventDisableTiming) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    // The mirror: the loop publishes the state after step `it` and looks at step it - 1's copy, so it enqueues a step
    // before it knows how the one before ended.  `bytes`: how much of the state the loop reads per step.
    bool publish(long long it, size_t bytes, hipStream_t s) {
        return hipMemcpyAsync(&pinned[it & 1], state, bytes, hipMemcpyDeviceToHost, s) == hipSuccess &&
               hipEventRecord(seen[it & 1], s) == hipSuccess;
    }
    const State& previous(long long it) const { return pinned[(it - 1) & 1]; }    // it >= 1
    // waits for the copy published at step it - 1 (it >= 1); nullptr when the wait fails
    const State* wait_previous(long long it) {
        return hipEventSynchronize(seen[(it - 1) & 1]) == hipSuccess ? &previous(it) : nullptr;
    }
    // `bytes` of the state into pinned[0], waited for: the read-back after setup and at the end.  `ok`: what the
    // calls before it came to.  false (and the HIP error cleared) when they or the copy failed.
    bool read_back(bool ok, hipStream_t s, size_t bytes = sizeof(State)) {
        ok = ok && hipMemcpyAsync(&pinned[0], state, bytes, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        return ok;
    }
    // The end of a timed loop: ev.stop, read_back of the whole state, the elapsed time into *elapsed_ms.
    bool finish_timed(bool ok, EventPair& ev, hipStream_t s, float* elapsed_ms) {
        ok = read_back(ok && hipEventRecord(ev.stop, s) == hipSuccess, s);
        float ms = 0.0f;
        if (ok && hipEventElapsedTime(&ms, ev.start, ev.stop) == hipSuccess) *elapsed_ms = ms;
        return ok;
    }
    ~Workspace() {
        if (vec) (void)hipFree(vec);
        if (part) (void)hipFree(part);
        if (state) (void)hipFree(state);
        if (pinned) (void)hipHostFree(pinned);
        for (hipEvent_t e : seen) if (e) (void)hipEventDestroy(e);
    }
};

constexpr int kRoundsPerBatch = 8;      // rounds enqueued between two looks at the count of vertices left

// The host loop of a Jones-Plassmann algorithm in rounds over n >= 1 vertices (csr_color, the MIS-2 aggregation).
// State, the device state `ws` mirrors, holds `int remaining[3]` (remaining[r % 3] = vertices still undecided after
// round r) and `int rounds` (rounds that found something to do); the round kernels keep both.  enqueue_round(r)
// enqueues round r = 0, 1, ... on `s` and returns its hipError_t.
// Batches of kRoundsPerBatch rounds, each followed by a copy of the state; batch b + 1 is enqueued before batch b's
// copy is looked at, and the last batch is waited for at once.  The highest-priority undecided vertex always decides,
// so n rounds are enough for any graph; a copy that shows fewer rounds than had been enqueued by then shows a round
// that found nothing to do, which ends the loop as remaining == 0 after the last counted round does.  false when a
// call fails.
template <class State, class EnqueueRound>
bool run_rounds(int n, Workspace<State>& ws, hipStream_t s, EnqueueRound&& enqueue_round) {
    int enqueued = 0;
    int enqueued_at[2] = {0, 0};
    bool ok = true, done = false;
    for (long long batch = 0; ok && !done; ++batch) {
        const int todo = std::min(kRoundsPerBatch, n - enqueued);
        for (int t = 0; t < todo && ok; ++t) {
            ok = enqueue_round(enqueued) == hipSuccess;
            ++enqueued;
        }
        enqueued_at[batch & 1] = enqueued;
        ok = ok && ws.publish(batch, sizeof(State), s);
        const bool last = enqueued >= n;
        const long long look = last ? batch + 1 : batch;          // the last batch is waited for at once
        if (ok && look >= 1) {
            const State* st = ws.wait_previous(look);
            ok = st != nullptr;
            if (ok) {
                const int seen_rounds = st->rounds;
                done = seen_rounds < enqueued_at[(look - 1) & 1] ||
                       (seen_rounds >= 1 && st->remaining[(seen_rounds - 1) % 3] == 0);
            }
            if (ok && last && !done) ok = false;                  // cannot happen: n rounds decide n vertices
        }
    }
    return ok;
}

// The LDS-tiled engine's part in one solve of A (pagerank()'s rule): engine 1 builds the plan at once, 0 never uses
// one, -1 takes a cached plan from the start, else builds one after 4 direct steps if A is eligible.
struct TiledEngine {
    enum class Spmv { TILED, DIRECT, FAILED };

    const CSRMatrix* A;
    PlanRef plan;
    int build_plan_at = -1;

    TiledEngine(const CSRMatrix* matrix, int engine, hipStream_t s) : A(matrix) {
        if (engine == 1) {
            plan = tiled_plan_for(A, s);
        } else if (engine == -1) {
            plan = tiled_plan_if_cached(A);
            if (!plan && tiled_eligible(A)) build_plan_at = 4;
        }
    }
    // Top of step `it`.  Once enough direct steps are paid: drains the queue (`ok`: whether that worked; no plan is
    // built when it did not), then builds the plan.  false: the mirror shows that the loop has already ended, nothing
    // is built for it and the loop ends here.
    template <class State>
    bool build_if_due(long long it, const Workspace<State>& ws, hipStream_t s, bool& ok) {
        if (plan || it != build_plan_at) return true;
        ok = hipStreamSynchronize(s) == hipSuccess;
        if (ok && it >= 1 && ws.previous(it).done) return false;
        if (ok) plan = tiled_plan_for(A, s);
        return true;
    }
    // y = A x on the tiled engine (ungated: y holds nothing live).  DIRECT: no plan is held, the caller runs its
    // direct kernel.  No tiled scratch for this stream (hipErrorOutOfMemory) drops the plan for good: DIRECT from
    // here on.
    Spmv spmv(const float* x, float* y, hipStream_t s) {
        if (!plan) return Spmv::DIRECT;
        const hipError_t e = tiled_spmv(*plan, x, y, s);
        if (e == hipSuccess) return Spmv::TILED;
        if (e != hipErrorOutOfMemory) return Spmv::FAILED;
        (void)hipGetLastError();
        plan.reset();
        build_plan_at = -1;
        return Spmv::DIRECT;
    }
};

} // namespace solver
} // namespace detail
} // namespace spmv

#endif
