// ic0_host.cpp — host side of the IC(0) factorisation (include/spmv/ic0.h): the host factorisation
// ic0_cpu_csr, which defines the arithmetic, and the device entry points over the LOWER schedule that sptrsv_host.cpp
// keeps with the matrix.  The kernels are in ic0.hip.  Built without FMA contraction: the fused multiply-adds below
// are the explicit std::fmaf calls and nothing else.
#include "internal.h"
#include "spmv/ic0.h"
#include "spmv/sptrsv.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace spmv {

int ic0_cpu_csr(const CSRMatrix* A, float* l_values, int* bad_pivot) {
    using detail::code;
    if (!A || !l_values) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) {
        if (bad_pivot) *bad_pivot = -1;
        return code(SpMVError::SUCCESS);
    }
    if (n < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
    // everything that can fail, before l_values is touched
    if (ptr[0] < 0 || ptr[n] > A->nnz) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {
        if (ptr[i + 1] < ptr[i]) return code(SpMVError::INVALID_FORMAT);
    }
    for (int j = ptr[0]; j < ptr[n]; ++j) {
        if (col[j] < 0 || col[j] >= n) return code(SpMVError::INVALID_FORMAT);
    }
    std::vector<int> diagonal(static_cast<size_t>(n), -1);      // position of (i,i)
    bool ascending = true;
    for (int i = 0; i < n; ++i) {
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (j > ptr[i] && col[j] <= col[j - 1]) ascending = false;
            if (col[j] == i) diagonal[i] = j;
        }
    }
    if (!ascending) return code(SpMVError::INVALID_ARGUMENT);
    for (int i = 0; i < n; ++i) {
        if (diagonal[i] < 0) return code(SpMVError::INVALID_ARGUMENT);
    }
    if (detail::one_sided_row(n, ptr, col) >= 0) return code(SpMVError::INVALID_ARGUMENT);

    float* l = l_values;
    const float* a = A->values;
    // next[k]: the upper position of row k that the next row below it with a stored (i,k) mirrors into.  The pattern
    // is symmetric and the rows run in ascending i, so that position is (k,i).
    std::vector<int> next(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) next[i] = diagonal[i] + 1;
    for (int i = 0; i < n; ++i) {
        const int di = diagonal[i];
        if (l != a) {
            for (int t = ptr[i]; t <= di; ++t) l[t] = a[t];
        }
        for (int pk = ptr[i]; pk < di; ++pk) {
            const int k = col[pk];
            const float lik = l[pk] / l[diagonal[k]];
            l[pk] = lik;
            // the stored j of row i with k < j < i that row k also stores: both rows ascend, one merge; l_jk is
            // read from (k,j), where row j put it when it finished
            int q = diagonal[k] + 1;
            const int q_end = ptr[k + 1];
            for (int t = pk + 1; t < di && q < q_end; ++t) {
                while (q < q_end && col[q] < col[t]) ++q;
                if (q < q_end && col[q] == col[t]) l[t] = std::fmaf(-lik, l[q], l[t]);
            }
            l[di] = std::fmaf(-lik, lik, l[di]);
            l[next[k]++] = lik;                                  // (k,i)
        }
        l[di] = std::sqrt(l[di]);
    }
    if (bad_pivot) {
        *bad_pivot = -1;
        for (int i = 0; i < n; ++i) {
            const float d = l[diagonal[i]];
            if (!(d > 0.0f && std::isfinite(d))) {
                *bad_pivot = i;
                break;
            }
        }
    }
    return code(SpMVError::SUCCESS);
}

namespace detail {
namespace {

using ScheduleRef = std::shared_ptr<const SptrsvSchedule>;

bool partial_overlap(const float* a, const float* b, long long count) {
    if (a == b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t bytes = static_cast<uintptr_t>(count) * sizeof(float);
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

int ic0_lanes_for(const SptrsvSchedule& s) {
    long long forced = 0;
    if (debug_option("ic0_lanes", &forced) && forced >= 1 && forced <= 64 && (forced & (forced - 1)) == 0) {
        return static_cast<int>(forced);
    }
    return pick_lanes_per_row(static_cast<float>(s.nnz) / static_cast<float>(s.num_rows));
}

// Everything before the launches.  On SUCCESS with *schedule null there is nothing to do (no rows).
int prepare(const CSRMatrix* A, const float* d_l, hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) {
    schedule->reset();
    *analysis_ms = 0.0f;
    if (!A || !d_l) return code(SpMVError::INVALID_ARGUMENT);
    bool nothing = false;
    const int status = sptrsv_check_matrix(A, &nothing);
    if (status != 0 || nothing) return status;
    if (partial_overlap(A->d_values, d_l, A->nnz)) return code(SpMVError::INVALID_ARGUMENT);
    ScheduleRef found;
    const int analysed = sptrsv_schedule_for(A, SpTRSVConfig::LOWER, stream, &found, analysis_ms);
    if (analysed != 0) return analysed;
    if (found->first_unsorted_row >= 0 || found->first_missing_diagonal >= 0 || found->one_sided_row >= 0) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    *schedule = found;
    return code(SpMVError::SUCCESS);
}

} // namespace
} // namespace detail

IC0Result ic0_csr(const CSRMatrix* A, float* d_l_values) {
    using namespace detail;
    IC0Result result;
    hipStream_t stream = current_stream();
    ScheduleRef schedule;
    result.error_code = prepare(A, d_l_values, stream, &schedule, &result.analysis_ms);
    if (result.error_code != 0 || !schedule) return result;

    const TraceRange range("spmv:ic0_csr");
    const int lanes = ic0_lanes_for(*schedule);
    result.num_levels = schedule->num_levels;
    result.launches = static_cast<int>(schedule->groups.size());
    result.lanes_per_row = lanes;
    unsigned* d_pivot = nullptr;       // lowest bad row as an unsigned minimum; all ones = none
    if (hipMalloc(reinterpret_cast<void**>(&d_pivot), sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::CUDA_MALLOC);
        return result;
    }
    EventPair& ev = thread_events();
    unsigned pivot = UINT_MAX;
    bool ok = hipMemsetAsync(d_pivot, 0xff, sizeof(unsigned), stream) == hipSuccess &&
              ev.start && ev.stop && hipEventRecord(ev.start, stream) == hipSuccess;
    ok = ok && launch_ic0(*schedule, A, A->d_values, d_l_values, lanes, d_pivot, stream) == hipSuccess;
    ok = ok && hipEventRecord(ev.stop, stream) == hipSuccess &&
         hipMemcpyAsync(&pivot, d_pivot, sizeof(unsigned), hipMemcpyDeviceToHost, stream) == hipSuccess;
    // always drained: `pivot` lives in this frame
    ok = (hipStreamSynchronize(stream) == hipSuccess) && ok && hipGetLastError() == hipSuccess &&
         hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) == hipSuccess;
    (void)hipFree(d_pivot);
    if (!ok) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::KERNEL_LAUNCH);
        return result;
    }
    result.bad_pivot = pivot == UINT_MAX ? -1 : static_cast<int>(pivot);
    return result;
}

int ic0_csr_async(const CSRMatrix* A, float* d_l_values, hipStream_t stream) {
    using namespace detail;
    ScheduleRef schedule;
    float analysis_ms = 0.0f;
    const int status = prepare(A, d_l_values, stream, &schedule, &analysis_ms);
    if (status != 0 || !schedule) return status;
    const hipError_t e = launch_ic0(*schedule, A, A->d_values, d_l_values, ic0_lanes_for(*schedule), nullptr, stream);
    return e == hipSuccess ? code(SpMVError::SUCCESS) : code(SpMVError::KERNEL_LAUNCH);
}

} // namespace spmv
