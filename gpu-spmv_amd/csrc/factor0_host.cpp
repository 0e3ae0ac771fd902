// factor0_host.cpp — host side of the zero-fill factorisations ILU(0) (include/spmv/ilu0.h) and
// IC(0) (include/spmv/ic0.h): the host factorisations ilu0_cpu_csr and ic0_cpu_csr, which define the
// arithmetic, and the device entry points over the LOWER schedule that sptrsv_host.cpp keeps with the matrix.  The
// kernels are in factor0.hip.  Built without FMA contraction: the fused multiply-adds below are the explicit
// std::fmaf calls and nothing else.
#include "internal.h"
#include "level_driver.h"
#include "spmv/ic0.h"
#include "spmv/ilu0.h"
#include "spmv/sptrsv.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace spmv {

namespace detail {
namespace {

// What ilu0_cpu_csr and ic0_cpu_csr check alike, in the order their callers rely on: everything that can fail,
// before `out` is touched.  On SUCCESS *diagonal holds the position of every (i,i); for a matrix without rows it
// stays empty, *pivot (may be null) is -1 and there is nothing to factor.
int check_cpu_factor(const CSRMatrix* A, const float* out, int* pivot, std::vector<int>* diagonal) {
    diagonal->clear();
    if (!A || !out) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) {
        if (pivot) *pivot = -1;
        return code(SpMVError::SUCCESS);
    }
    if (n < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
    if (ptr[0] < 0 || ptr[n] > A->nnz) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {
        if (ptr[i + 1] < ptr[i]) return code(SpMVError::INVALID_FORMAT);
    }
    for (int j = ptr[0]; j < ptr[n]; ++j) {
        if (col[j] < 0 || col[j] >= n) return code(SpMVError::INVALID_FORMAT);
    }
    std::vector<int> found(static_cast<size_t>(n), -1);         // position of (i,i)
    bool ascending = true;
    for (int i = 0; i < n; ++i) {
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (j > ptr[i] && col[j] <= col[j - 1]) ascending = false;
            if (col[j] == i) found[i] = j;
        }
    }
    if (!ascending) return code(SpMVError::INVALID_ARGUMENT);
    for (int i = 0; i < n; ++i) {
        if (found[i] < 0) return code(SpMVError::INVALID_ARGUMENT);
    }
    diagonal->swap(found);
    return code(SpMVError::SUCCESS);
}

} // namespace
} // namespace detail

int ilu0_cpu_csr(const CSRMatrix* A, float* lu_values, int* zero_pivot) {
    using detail::code;
    std::vector<int> diagonal;
    const int checked = detail::check_cpu_factor(A, lu_values, zero_pivot, &diagonal);
    if (checked != 0 || diagonal.empty()) return checked;
    const int n = A->num_rows;
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;

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

int ic0_cpu_csr(const CSRMatrix* A, float* l_values, int* bad_pivot) {
    using detail::code;
    std::vector<int> diagonal;
    const int checked = detail::check_cpu_factor(A, l_values, bad_pivot, &diagonal);
    if (checked != 0 || diagonal.empty()) return checked;
    const int n = A->num_rows;
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
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

// ilu0_csr / ic0_csr and their async forms as an Op of level_driver.h
struct CsrFactor {
    Factor0Kind kind;
    const CSRMatrix* A;
    float* d_out;
    int prepare(hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) const {
        schedule->reset();
        *analysis_ms = 0.0f;
        if (!A || !d_out) return code(SpMVError::INVALID_ARGUMENT);
        bool nothing = false;
        const int status = sptrsv_check_matrix(A, &nothing);
        if (status != 0 || nothing) return status;
        if (partial_overlap(A->d_values, d_out, A->nnz)) return code(SpMVError::INVALID_ARGUMENT);
        ScheduleRef found;
        const int analysed = sptrsv_schedule_for(A, SpTRSVConfig::LOWER, stream, &found, analysis_ms);
        if (analysed != 0) return analysed;
        if (found->first_unsorted_row >= 0 || found->first_missing_diagonal >= 0 ||
            (kind == Factor0Kind::IC0 && found->one_sided_row >= 0)) {
            return code(SpMVError::INVALID_ARGUMENT);
        }
        *schedule = found;
        return code(SpMVError::SUCCESS);
    }
    int lanes(const SptrsvSchedule& s) const {
        if (int f = forced_lanes(kind == Factor0Kind::IC0 ? "ic0_lanes" : "ilu0_lanes")) return f;
        return pick_lanes_per_row(static_cast<float>(s.nnz) / static_cast<float>(s.num_rows));
    }
    // d_pivot null: the launches alone, no pivot scan
    hipError_t launch(const SptrsvSchedule& schedule, int lanes, hipStream_t stream, unsigned* d_pivot) const {
        return launch_factor0(kind, schedule, A, A->d_values, d_out, lanes, d_pivot, stream);
    }
};

} // namespace
} // namespace detail

ILU0Result ilu0_csr(const CSRMatrix* A, float* d_lu_values) {
    using namespace detail;
    return factor_result(timed_factor("spmv:ilu0_csr", CsrFactor{Factor0Kind::ILU0, A, d_lu_values}),
                         &ILU0Result::zero_pivot);
}

IC0Result ic0_csr(const CSRMatrix* A, float* d_l_values) {
    using namespace detail;
    return factor_result(timed_factor("spmv:ic0_csr", CsrFactor{Factor0Kind::IC0, A, d_l_values}),
                         &IC0Result::bad_pivot);
}

int ilu0_csr_async(const CSRMatrix* A, float* d_lu_values, hipStream_t stream) {
    using namespace detail;
    return launch_factor_async(CsrFactor{Factor0Kind::ILU0, A, d_lu_values}, stream);
}

int ic0_csr_async(const CSRMatrix* A, float* d_l_values, hipStream_t stream) {
    using namespace detail;
    return launch_factor_async(CsrFactor{Factor0Kind::IC0, A, d_l_values}, stream);
}

} // namespace spmv
