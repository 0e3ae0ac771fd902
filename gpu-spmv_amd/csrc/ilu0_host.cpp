// ilu0_host.cpp — host side of the ILU(0) factorisation (include/spmv/ilu0.h): the host
// factorisation ilu0_cpu_csr, which defines the arithmetic, and the device entry points over the LOWER schedule that
// sptrsv_host.cpp keeps with the matrix.  The kernels are in ilu0.hip.  Built without FMA contraction: the fused
// multiply-adds below are the explicit std::fmaf calls and nothing else.
#include "internal.h"
#include "spmv/ilu0.h"
#include "spmv/sptrsv.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace spmv {

int ilu0_cpu_csr(const CSRMatrix* A, float* lu_values, int* zero_pivot) {
    using detail::code;
    if (!A || !lu_values) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) {
        if (zero_pivot) *zero_pivot = -1;
        return code(SpMVError::SUCCESS);
    }
    if (n < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
    // everything that can fail, before lu_values is touched
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

    float* lu = lu_values;
    if (lu != A->values) std::memmove(lu, A->values, static_cast<size_t>(A->nnz) * sizeof(float));
    for (int i = 0; i < n; ++i) {
        for (int pk = ptr[i]; pk < diagonal[i]; ++pk) {
            const int k = col[pk];
            const float l = lu[pk] / lu[diagonal[k]];
            lu[pk] = l;
            // the stored j > k of row i that row k also stores: both rows ascend, one merge
            int q = diagonal[k] + 1;
            const int q_end = ptr[k + 1];
            for (int t = pk + 1; t < ptr[i + 1] && q < q_end; ++t) {
                while (q < q_end && col[q] < col[t]) ++q;
                if (q < q_end && col[q] == col[t]) lu[t] = std::fmaf(-l, lu[q], lu[t]);
            }
        }
    }
    if (zero_pivot) {
        *zero_pivot = -1;
        for (int i = 0; i < n; ++i) {
            const float u = lu[diagonal[i]];
            if (!(u != 0.0f && std::isfinite(u))) {
                *zero_pivot = i;
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

int ilu0_lanes_for(const SptrsvSchedule& s) {
    long long forced = 0;
    if (debug_option("ilu0_lanes", &forced) && forced >= 1 && forced <= 64 && (forced & (forced - 1)) == 0) {
        return static_cast<int>(forced);
    }
    return pick_lanes_per_row(static_cast<float>(s.nnz) / static_cast<float>(s.num_rows));
}

// Everything before the launches.  On SUCCESS with *schedule null there is nothing to do (no rows).
int prepare(const CSRMatrix* A, const float* d_lu, hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) {
    schedule->reset();
    *analysis_ms = 0.0f;
    if (!A || !d_lu) return code(SpMVError::INVALID_ARGUMENT);
    bool nothing = false;
    const int status = sptrsv_check_matrix(A, &nothing);
    if (status != 0 || nothing) return status;
    if (partial_overlap(A->d_values, d_lu, A->nnz)) return code(SpMVError::INVALID_ARGUMENT);
    ScheduleRef found;
    const int analysed = sptrsv_schedule_for(A, SpTRSVConfig::LOWER, stream, &found, analysis_ms);
    if (analysed != 0) return analysed;
    if (found->first_unsorted_row >= 0 || found->first_missing_diagonal >= 0) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    *schedule = found;
    return code(SpMVError::SUCCESS);
}

} // namespace
} // namespace detail

ILU0Result ilu0_csr(const CSRMatrix* A, float* d_lu_values) {
    using namespace detail;
    ILU0Result result;
    hipStream_t stream = current_stream();
    ScheduleRef schedule;
    result.error_code = prepare(A, d_lu_values, stream, &schedule, &result.analysis_ms);
    if (result.error_code != 0 || !schedule) return result;

    const TraceRange range("spmv:ilu0_csr");
    const int lanes = ilu0_lanes_for(*schedule);
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
    ok = ok && launch_ilu0(*schedule, A, A->d_values, d_lu_values, lanes, d_pivot, stream) == hipSuccess;
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
    result.zero_pivot = pivot == UINT_MAX ? -1 : static_cast<int>(pivot);
    return result;
}

int ilu0_csr_async(const CSRMatrix* A, float* d_lu_values, hipStream_t stream) {
    using namespace detail;
    ScheduleRef schedule;
    float analysis_ms = 0.0f;
    const int status = prepare(A, d_lu_values, stream, &schedule, &analysis_ms);
    if (status != 0 || !schedule) return status;
    const hipError_t e = launch_ilu0(*schedule, A, A->d_values, d_lu_values, ilu0_lanes_for(*schedule), nullptr,
                                     stream);
    return e == hipSuccess ? code(SpMVError::SUCCESS) : code(SpMVError::KERNEL_LAUNCH);
}

} // namespace spmv
