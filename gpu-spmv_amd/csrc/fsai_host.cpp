// fsai_host.cpp — host side of the factorised sparse approximate inverse (include/spmv/fsai.h):
// fsai_cpu_csr, which defines the arithmetic, and the drivers of fsai_csr and fsai_csr_numeric over the kernels of
// fsai.hip.  Built without FMA contraction: the fused multiply-adds are fsai_impl.h's explicit std::fma calls and
// nothing else.
#include "internal.h"
#include "fsai_impl.h"
#include "spmv/fsai.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace spmv {

namespace detail {
namespace fsai {
namespace {

// What every entry point checks before it looks at an array: *pattern is S, or A where S is null; *nothing_to_do when
// the matrix has no rows.
int check_shapes(const CSRMatrix* G, const CSRMatrix* A, const CSRMatrix* S, const CSRMatrix** pattern,
                 bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!G || !A) return code(SpMVError::INVALID_ARGUMENT);
    *pattern = S ? S : A;
    if (G == A || G == *pattern) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if ((*pattern)->num_rows != (*pattern)->num_cols || (*pattern)->num_rows != A->num_rows) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    *nothing_to_do = A->num_rows == 0;
    return code(SpMVError::SUCCESS);
}

// the host arrays of a square matrix: 0, or the code of the first rule of fsai.h's list that they break
int check_host_structure(const CSRMatrix* M, bool need_values, bool* unsorted) {
    const int n = M->num_rows;
    if (n < 0 || M->nnz < 0 || !M->row_ptrs || (M->nnz > 0 && (!M->col_indices || (need_values && !M->values)))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    for (int i = 0; i < n; ++i) {
        const int b = M->row_ptrs[i], e = M->row_ptrs[i + 1];
        if (b < 0 || e > M->nnz || b > e) return code(SpMVError::INVALID_FORMAT);
        for (int t = b; t < e; ++t) {
            const int c = M->col_indices[t];
            if (c < 0 || c >= n) return code(SpMVError::INVALID_FORMAT);
            if (t > b && c <= M->col_indices[t - 1]) *unsorted = true;
        }
    }
    return code(SpMVError::SUCCESS);
}

// row i of G on the pattern P[0, m), P[m - 1] == i, from A's host arrays: the rule of fsai.h with T and U as the
// kernel's slab
void host_row(const CSRMatrix* A, const int* P, int m, double* T, double* U, float* g) {
    std::fill(T, T + tri(m, 0), 0.0);
    std::fill(U, U + m, 0.0);
    for (int p = 0; p < m; ++p) {
        const int j = P[p];
        int q = 0;
        for (int t = A->row_ptrs[j]; t < A->row_ptrs[j + 1]; ++t) {
            const int c = A->col_indices[t];
            if (c > j) break;
            while (q <= p && P[q] < c) ++q;
            if (q > p) break;
            if (P[q] == c) T[tri(p, q)] = static_cast<double>(A->values[t]);
        }
    }
    for (int q = 0; q < m; ++q) {
        const double cqq = sqrt_rn(cholesky_w(T, q, q));
        T[tri(q, q)] = cqq;
        for (int p = q + 1; p < m; ++p) T[tri(p, q)] = div_rn(cholesky_w(T, p, q), cqq);
    }
    for (int q = m - 1; q >= 0; --q) {
        U[q] = substitution_u(U[q], T[tri(q, q)], q == m - 1);
        for (int p = 0; p < q; ++p) U[p] = substitution_t(T[tri(q, p)], U[q], U[p]);
    }
    for (int p = 0; p < m; ++p) g[p] = static_cast<float>(U[p]);
}

// neither rule of internal.h: nnz < 0 fails, num_rows is the caller's to check, and a pattern needs no values
bool structure_on_device(const CSRMatrix* M) {
    return M->nnz >= 0 && M->d_row_ptrs && (M->nnz == 0 || M->d_col_indices);
}
bool arrays_on_device(const CSRMatrix* M) { return structure_on_device(M) && (M->nnz == 0 || M->d_values); }

// the class and the lanes of one call: 0 when a forced class is too small for max_row
int pick_class(int max_row) {
    long long forced = 0;
    if (debug_option("fsai_class", &forced) && is_class(forced)) {
        return forced >= max_row ? static_cast<int>(forced) : 0;
    }
    return class_for(max_row);
}
int pick_lanes(int max_row) {
    if (int f = forced_lanes("fsai_lanes")) return f;
    int lanes = 1;                       // lane p gathers row j_p: one lane per entry of the longest row
    while (lanes < max_row) lanes <<= 1;
    return std::min(lanes, 64);
}

FSAIResult failed(FSAIResult result, SpMVError e) {
    (void)hipGetLastError();
    result.error_code = code(e);
    return result;
}

} // namespace
} // namespace fsai
} // namespace detail

int fsai_cpu_csr(CSRMatrix* G, const CSRMatrix* A, const CSRMatrix* S, int* bad_row) {
    using namespace detail::fsai;
    using detail::code;
    const CSRMatrix* pattern = nullptr;
    bool nothing = false;
    const int shapes = check_shapes(G, A, S, &pattern, &nothing);
    if (shapes != 0) return shapes;
    const int n = A->num_rows;
    std::vector<int> row_ptrs(static_cast<size_t>(std::max(n, 0)) + 1, 0);
    std::vector<int> cols;
    std::vector<float> vals;
    int bad = -1;
    if (!nothing) {
        bool unsorted = false;
        int status = check_host_structure(A, true, &unsorted);
        if (status == 0 && pattern != A) status = check_host_structure(pattern, false, &unsorted);
        if (status != 0) return status;
        if (unsorted) return code(SpMVError::INVALID_ARGUMENT);
        bool long_row = false;
        for (int i = 0; i < n; ++i) {
            bool diagonal = false;
            for (int t = pattern->row_ptrs[i]; t < pattern->row_ptrs[i + 1] && pattern->col_indices[t] <= i; ++t) {
                cols.push_back(pattern->col_indices[t]);
                diagonal = pattern->col_indices[t] == i;
            }
            if (!diagonal) return code(SpMVError::INVALID_ARGUMENT);
            row_ptrs[i + 1] = static_cast<int>(cols.size());
            long_row = long_row || row_ptrs[i + 1] - row_ptrs[i] > kFsaiMaxRow;
        }
        if (long_row) return code(SpMVError::INVALID_ARGUMENT);
        vals.resize(cols.size());
        std::vector<double> T(static_cast<size_t>(tri(kFsaiMaxRow, 0))), U(kFsaiMaxRow);
        for (int i = 0; i < n; ++i) {
            const int b = row_ptrs[i], m = row_ptrs[i + 1] - b;
            host_row(A, cols.data() + b, m, T.data(), U.data(), vals.data() + b);
            const float d = vals[b + m - 1];
            if (bad < 0 && !(d > 0.0f && std::isfinite(d))) bad = i;
        }
    }
    detail::csr_adopt_host(G, n, n, row_ptrs, cols, vals);
    if (bad_row) *bad_row = bad;
    return code(SpMVError::SUCCESS);
}

FSAIResult fsai_csr(CSRMatrix* G, const CSRMatrix* A, const CSRMatrix* S) {
    using namespace detail;
    using namespace detail::fsai;
    FSAIResult result;
    const CSRMatrix* pattern = nullptr;
    bool nothing = false;
    result.error_code = check_shapes(G, A, S, &pattern, &nothing);
    if (result.error_code != 0) return result;
    const int n = A->num_rows;
    if (n < 0 || (!nothing && (!arrays_on_device(A) || !structure_on_device(pattern)))) {
        return failed(result, SpMVError::INVALID_FORMAT);
    }
    hipStream_t stream = current_stream();
    if (nothing) {
        DeviceCsrArrays empty;
        const ReleaseOnExit release_empty{&empty};
        if (empty.alloc(1, 0) != hipSuccess) return failed(result, SpMVError::CUDA_MALLOC);
        if (hipMemsetAsync(empty.row_ptrs, 0, sizeof(int), stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            return failed(result, SpMVError::KERNEL_LAUNCH);
        }
        csr_adopt_device(G, 0, 0, 0, &empty);
        return result;
    }

    const TraceRange range("spmv:fsai_csr");
    // ---- structure: counts -> row pointers, and the one read-back ----
    const std::vector<long long> levels = device_scan_levels(static_cast<long long>(n) + 1);
    DeviceCsrArrays g;
    const ReleaseOnExit release_g{&g};
    DevBuf<int> sums;
    DevBuf<unsigned> info, word;         // kInfoWords of the structure pass; the bad_row word, kept with G
    if (g.alloc(static_cast<long long>(n) + 1, 0) != hipSuccess ||
        dev_alloc(&sums, device_scan_sums(levels)) != hipSuccess || dev_alloc(&info, kInfoWords) != hipSuccess ||
        dev_alloc(&word, 1) != hipSuccess) {
        return failed(result, SpMVError::CUDA_MALLOC);
    }
    EventPair& ev = thread_events();
    unsigned seen[kInfoWords] = {0, 0, 0, 0, 0};
    int g_nnz = 0;
    bool ok = ev.start && ev.stop && hipEventRecord(ev.start, stream) == hipSuccess &&
              hipMemsetAsync(info.get(), 0, kInfoWords * sizeof(unsigned), stream) == hipSuccess &&
              hipMemsetAsync(info.get() + kLongRow, 0xff, sizeof(unsigned), stream) == hipSuccess &&
              hipMemsetAsync(word.get(), 0xff, sizeof(unsigned), stream) == hipSuccess;
    ok = ok && launch_structure_count(A, pattern, g.row_ptrs, info.get(), stream) == hipSuccess &&
         device_exclusive_scan(g.row_ptrs, levels, sums.get(), stream) == hipSuccess &&
         hipMemcpyAsync(seen, info.get(), sizeof(seen), hipMemcpyDeviceToHost, stream) == hipSuccess &&
         hipMemcpyAsync(&g_nnz, g.row_ptrs + n, sizeof(int), hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok;       // always drained: `seen` lives in this frame
    if (!ok) return failed(result, SpMVError::KERNEL_LAUNCH);
    if (seen[kBadFormat]) return failed(result, SpMVError::INVALID_FORMAT);
    if (seen[kUnsorted] || seen[kNoDiagonal]) return failed(result, SpMVError::INVALID_ARGUMENT);
    result.max_row = static_cast<int>(seen[kMaxRow]);
    if (seen[kLongRow] != UINT_MAX) {
        result.long_row = static_cast<int>(seen[kLongRow]);
        return failed(result, SpMVError::INVALID_ARGUMENT);
    }
    result.row_class = pick_class(result.max_row);
    if (result.row_class == 0) return failed(result, SpMVError::INVALID_ARGUMENT);
    result.lanes_per_row = pick_lanes(result.max_row);
    result.nnz = g_nnz;

    // ---- the columns and the values ----
    if (g.alloc_entries(g_nnz) != hipSuccess) return failed(result, SpMVError::CUDA_MALLOC);    // (g_nnz >= n >= 1)
    unsigned bad = UINT_MAX;
    ok = launch_structure_columns(pattern, g.row_ptrs, g.col_indices, stream) == hipSuccess &&
         launch_numeric(A, n, g_nnz, g.row_ptrs, g.col_indices, g.values, result.row_class,
                        result.lanes_per_row, word.get(), stream) == hipSuccess &&
         hipEventRecord(ev.stop, stream) == hipSuccess &&
         hipMemcpyAsync(&bad, word.get(), sizeof(unsigned), hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok && hipGetLastError() == hipSuccess &&
         hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) == hipSuccess;
    if (!ok) return failed(result, SpMVError::KERNEL_LAUNCH);
    result.bad_row = bad == UINT_MAX ? -1 : static_cast<int>(bad);

    csr_adopt_device(G, n, n, g_nnz, &g);
    CsrAux* aux = aux_lookup(G->d_row_ptrs, true);
    aux->fsai_max_row = result.max_row;
    if (aux->d_fsai_word) (void)hipFree(aux->d_fsai_word);
    aux->d_fsai_word = word.release();
    return result;
}

FSAIResult fsai_csr_numeric(CSRMatrix* G, const CSRMatrix* A) {
    using namespace detail;
    using namespace detail::fsai;
    FSAIResult result;
    if (!G || !A || G == A) return failed(result, SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols || G->num_rows != G->num_cols || G->num_rows != A->num_rows) {
        return failed(result, SpMVError::INVALID_DIMENSION);
    }
    const int n = A->num_rows;
    if (n == 0) return result;
    if (n < 0 || !arrays_on_device(A) || !arrays_on_device(G) || G->nnz == 0) {
        return failed(result, SpMVError::INVALID_FORMAT);
    }
    hipStream_t stream = current_stream();
    // what fsai_csr left with G; a G from elsewhere has its rows measured, and its word allocated, once
    CsrAux* aux = aux_lookup(G->d_row_ptrs, true);
    if (aux->fsai_max_row <= 0) {
        int longest = 0, shortest = 0;
        if (device_row_stats(G->d_row_ptrs, n, &longest, &shortest, stream) != hipSuccess) {
            return failed(result, SpMVError::KERNEL_LAUNCH);
        }
        aux->fsai_max_row = longest;
    }
    if (!aux->d_fsai_word && hipMalloc(reinterpret_cast<void**>(&aux->d_fsai_word), sizeof(unsigned)) != hipSuccess) {
        aux->d_fsai_word = nullptr;
        return failed(result, SpMVError::CUDA_MALLOC);
    }
    result.max_row = aux->fsai_max_row;
    result.nnz = G->nnz;
    if (result.max_row > kFsaiMaxRow) return failed(result, SpMVError::INVALID_ARGUMENT);
    result.row_class = pick_class(result.max_row);
    if (result.row_class == 0) return failed(result, SpMVError::INVALID_ARGUMENT);
    result.lanes_per_row = pick_lanes(result.max_row);

    const TraceRange range("spmv:fsai_csr_numeric");
    EventPair& ev = thread_events();
    unsigned bad = UINT_MAX;
    bool ok = ev.start && ev.stop && hipEventRecord(ev.start, stream) == hipSuccess &&
              hipMemsetAsync(aux->d_fsai_word, 0xff, sizeof(unsigned), stream) == hipSuccess;
    ok = ok && launch_numeric(A, n, G->nnz, G->d_row_ptrs, G->d_col_indices, G->d_values, result.row_class,
                              result.lanes_per_row, aux->d_fsai_word, stream) == hipSuccess &&
         hipEventRecord(ev.stop, stream) == hipSuccess &&
         hipMemcpyAsync(&bad, aux->d_fsai_word, sizeof(unsigned), hipMemcpyDeviceToHost, stream) == hipSuccess;
    ok = hipStreamSynchronize(stream) == hipSuccess && ok && hipGetLastError() == hipSuccess &&
         hipEventElapsedTime(&result.elapsed_ms, ev.start, ev.stop) == hipSuccess;
    if (!ok) return failed(result, SpMVError::KERNEL_LAUNCH);
    result.bad_row = bad == UINT_MAX ? -1 : static_cast<int>(bad);
    return result;
}

} // namespace spmv
