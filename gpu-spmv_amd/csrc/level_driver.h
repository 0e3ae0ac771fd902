// level_driver.h — what the drivers over a level schedule share (sptrsv_host.cpp, factor0_host.cpp, bsr_tri_host.cpp;
// DESIGN.md §4.11 "level layer"): the argument predicates, the copy of a schedule's counts into a result, and the
// blocking, async and analyze shapes of an entry point.  Host code only, templates and inline functions: every
// driver file compiles its own copy, also when it is built stand-alone for the sanitized host programs.
//
// An Op is one solve or factorisation, a small struct of the entry point's arguments with
//   int prepare(hipStream_t, ScheduleRef*, float* analysis_ms) const
//       every check before the launches, in the entry point's own order, then the cached schedule.  SUCCESS with the
//       schedule left null: nothing to do (no rows).
//   int lanes(const SptrsvSchedule&) const
//   hipError_t launch(const SptrsvSchedule&, int lanes, hipStream_t) const                      a solve
//   hipError_t launch(const SptrsvSchedule&, int lanes, hipStream_t, unsigned* d_pivot) const   a factorisation
//       d_pivot null: the launches alone, no pivot word
#ifndef SPMV_AMD_LEVEL_DRIVER_H
#define SPMV_AMD_LEVEL_DRIVER_H

#include "internal.h"
#include "spmv/sptrsv.h"

#include <climits>
#include <cstdint>
#include <memory>

namespace spmv {
namespace detail {

// the floats [a, a + na) and [b, b + nb) share a byte
inline bool spans_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) &&
           b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}
// [a, a + count) and [b, b + count) overlap without being the same array (in place is allowed)
inline bool partial_overlap(const float* a, const float* b, long long count) {
    return a != b && spans_overlap(a, count, b, count);
}

inline bool uplo_ok(int uplo) { return uplo == SpTRSVConfig::LOWER || uplo == SpTRSVConfig::UPPER; }
inline bool diag_ok(int diag) { return diag == SpTRSVConfig::NON_UNIT || diag == SpTRSVConfig::UNIT; }
inline bool config_ok(const SpTRSVConfig& cfg) {
    return uplo_ok(cfg.uplo) && diag_ok(cfg.diag) && (cfg.ordered == 0 || cfg.ordered == 1);
}
inline SpTRSVConfig config_or_default(const SpTRSVConfig* config) { return config ? *config : SpTRSVConfig(); }

// num_levels and launches of any result or info struct
template <class Result>
void copy_counts(const SptrsvSchedule& schedule, Result* out) {
    out->num_levels = schedule.num_levels;
    out->launches = static_cast<int>(schedule.groups.size());
}

// The blocking, timed solve: device-event time of the launches alone, waited for on the stop event.
template <class Op>
SpTRSVResult timed_solve(const char* trace_name, const Op& op) {
    SpTRSVResult result;
    hipStream_t stream = current_stream();
    ScheduleRef schedule;
    result.error_code = op.prepare(stream, &schedule, &result.analysis_ms);
    if (result.error_code != 0 || !schedule) return result;

    const TraceRange range(trace_name);
    copy_counts(*schedule, &result);
    result.lanes_per_row = op.lanes(*schedule);
    EventPair& ev = thread_events();
    if (!ev.start || !ev.stop || hipEventRecord(ev.start, stream) != hipSuccess) {
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
        return result;
    }
    const hipError_t launched = op.launch(*schedule, result.lanes_per_row, stream);
    const hipError_t recorded = hipEventRecord(ev.stop, stream);
    const hipError_t waited = hipEventSynchronize(ev.stop);
    if (launched != hipSuccess || recorded != hipSuccess || waited != hipSuccess || hipGetLastError() != hipSuccess ||
        hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) != hipSuccess) {
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
    }
    return result;
}

// what ilu0_csr, ic0_csr and bsr_ic0 report, under the names they share
struct Factor0Run {
    int error_code = 0;
    int num_levels = 0, launches = 0, lanes_per_row = 0;
    int pivot = -1;                    // lowest (block) row with a bad pivot, or -1
    float analysis_ms = 0.0f, elapsed_ms = 0.0f;
};

// The blocking, timed factorisation with its pivot word: the stream is drained, since the word is read back.
template <class Op>
Factor0Run timed_factor(const char* trace_name, const Op& op) {
    Factor0Run result;
    hipStream_t stream = current_stream();
    ScheduleRef schedule;
    result.error_code = op.prepare(stream, &schedule, &result.analysis_ms);
    if (result.error_code != 0 || !schedule) return result;

    const TraceRange range(trace_name);
    copy_counts(*schedule, &result);
    result.lanes_per_row = op.lanes(*schedule);
    DevBuf<unsigned> d_pivot;          // lowest bad row as an unsigned minimum; all ones = none
    if (dev_alloc(&d_pivot, 1) != hipSuccess) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::CUDA_MALLOC);
        return result;
    }
    EventPair& ev = thread_events();
    unsigned pivot = UINT_MAX;
    bool ok = hipMemsetAsync(d_pivot.get(), 0xff, sizeof(unsigned), stream) == hipSuccess &&
              ev.start && ev.stop && hipEventRecord(ev.start, stream) == hipSuccess;
    ok = ok && op.launch(*schedule, result.lanes_per_row, stream, d_pivot.get()) == hipSuccess;
    ok = ok && hipEventRecord(ev.stop, stream) == hipSuccess &&
         hipMemcpyAsync(&pivot, d_pivot.get(), sizeof(unsigned), hipMemcpyDeviceToHost, stream) == hipSuccess;
    // always drained: `pivot` lives in this frame
    ok = (hipStreamSynchronize(stream) == hipSuccess) && ok && hipGetLastError() == hipSuccess &&
         hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
        return result;
    }
    result.pivot = pivot == UINT_MAX ? -1 : static_cast<int>(pivot);
    return result;
}

// a Factor0Run as the entry point's own result struct; `pivot` names its pivot member
template <class Result>
Result factor_result(const Factor0Run& run, int Result::*pivot) {
    Result result;
    result.error_code = run.error_code;
    result.num_levels = run.num_levels;
    result.launches = run.launches;
    result.lanes_per_row = run.lanes_per_row;
    result.*pivot = run.pivot;
    result.analysis_ms = run.analysis_ms;
    result.elapsed_ms = run.elapsed_ms;
    return result;
}

// The async shape: the launches alone on the caller's stream, nothing timed, nothing read back.  `more` is what the
// Op's launch takes after the stream: nothing for a solve, the (null) pivot word for a factorisation.
template <class Op, class... More>
int launch_async(const Op& op, hipStream_t stream, More... more) {
    ScheduleRef schedule;
    float analysis_ms = 0.0f;
    const int status = op.prepare(stream, &schedule, &analysis_ms);
    if (status != 0 || !schedule) return status;
    const hipError_t e = op.launch(*schedule, op.lanes(*schedule), stream, more...);
    return e == hipSuccess ? code(SpMVError::SUCCESS) : code(SpMVError::KERNEL_LAUNCH);
}
template <class Op>
int launch_factor_async(const Op& op, hipStream_t stream) {
    return launch_async(op, stream, static_cast<unsigned*>(nullptr));
}

// The analyze shape: check(&nothing_to_do) is the entry point's matrix checks, then uplo, then
// schedule_for(stream, &schedule, &analysis_ms) builds or finds the schedule.
template <class Check, class ScheduleFor>
SpTRSVResult analyze_levels(int uplo, Check&& check, ScheduleFor&& schedule_for) {
    SpTRSVResult result;
    bool nothing = false;
    result.error_code = check(&nothing);
    if (result.error_code != 0 || nothing) return result;
    if (!uplo_ok(uplo)) {
        result.error_code = code(SpMVError::INVALID_ARGUMENT);
        return result;
    }
    ScheduleRef schedule;
    result.error_code = schedule_for(current_stream(), &schedule, &result.analysis_ms);
    if (result.error_code == 0) copy_counts(*schedule, &result);
    return result;
}

} // namespace detail
} // namespace spmv

#endif
