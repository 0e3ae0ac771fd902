// amg_host.cpp — the setup of the aggregation AMG (include/spmv/amg.h): argument checks, the host
// aggregation (amg_aggregate_cpu_csr is its definition), the Galerkin products through csr_transpose_gpu and
// spgemm_csr, the diagonals, and the fp64 Cholesky inverse of the coarsest level.  Setup runs once per matrix and is
// not the hot path; the V-cycle's kernels are in amg.hip.  amg_setup_smoothed shares the builder: its coarsening step
// is detail::amg_smooth_coarsen (amg_setup.hip), and amg_prolongator_cpu_csr here is that step's P on host arrays.
#include "amg_impl.h"
#include "internal.h"
#include "spmv/csr_ops.h"
#include "spmv/spgemm.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace spmv {

namespace {

using detail::code;

using detail::amg_diagonal;
using detail::amg_strong;
using detail::amg_structure_ok;

// the three passes of amg.h on a valid structure; returns the number of aggregates
int aggregate(int n, const int* rp, const int* ci, const float* va, float theta, int* agg) {
    std::vector<float> d;
    amg_diagonal(n, rp, ci, va, &d, nullptr);
    const double t2 = static_cast<double>(theta) * static_cast<double>(theta);
    const auto strong = [&](int i, int p) { return amg_strong(i, ci[p], va[p], t2, d[i], d[ci[p]]); };
    for (int i = 0; i < n; ++i) agg[i] = -1;
    int next = 0;
    for (int i = 0; i < n; ++i) {
        if (agg[i] != -1) continue;
        bool all_free = true;
        for (int p = rp[i]; p < rp[i + 1] && all_free; ++p) {
            if (strong(i, p) && agg[ci[p]] != -1) all_free = false;
        }
        if (!all_free) continue;
        agg[i] = next;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (strong(i, p)) agg[ci[p]] = next;
        }
        ++next;
    }
    const std::vector<int> after_first(agg, agg + n);
    for (int i = 0; i < n; ++i) {
        if (after_first[i] != -1) continue;
        int best = -1;
        float best_abs = 0.0f;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (!strong(i, p) || after_first[ci[p]] == -1) continue;
            const float a = std::fabs(va[p]);
            if (best == -1 || a > best_abs) {
                best = ci[p];
                best_abs = a;
            }
        }
        if (best != -1) agg[i] = after_first[best];
    }
    for (int i = 0; i < n; ++i) {
        if (agg[i] != -1) continue;
        agg[i] = next;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (strong(i, p) && agg[ci[p]] == -1) agg[ci[p]] = next;
        }
        ++next;
    }
    return next;
}

// The inverse of the SPD matrix given by its entries (duplicates add up, in fp64), by Cholesky in fp64 from the lower
// triangle; symmetric by construction (the upper triangle of Linv^T Linv, mirrored), rounded to fp32.  Returns the row
// of the first pivot that is not > 0, or -1.
int dense_inverse(int n, const int* rp, const int* ci, const float* va, std::vector<float>* out) {
    const size_t N = static_cast<size_t>(n);
    std::vector<double> L(N * N, 0.0);
    for (int i = 0; i < n; ++i) {
        for (int p = rp[i]; p < rp[i + 1]; ++p) L[i * N + ci[p]] += static_cast<double>(va[p]);
    }
    for (size_t j = 0; j < N; ++j) {
        double s = L[j * N + j];
        for (size_t k = 0; k < j; ++k) s -= L[j * N + k] * L[j * N + k];
        if (!(s > 0.0) || !std::isfinite(s)) return static_cast<int>(j);
        const double pivot = std::sqrt(s);
        L[j * N + j] = pivot;
        for (size_t i = j + 1; i < N; ++i) {
            double t = L[i * N + j];
            for (size_t k = 0; k < j; ++k) t -= L[i * N + k] * L[j * N + k];
            L[i * N + j] = t / pivot;
        }
    }
    // U = (L^-1)^T, row c of U = column c of L^-1 ... stored so that the final products run over contiguous rows:
    // U[c * N + i] = Linv[i][c], i >= c
    std::vector<double> U(N * N, 0.0);
    for (size_t c = 0; c < N; ++c) {
        U[c * N + c] = 1.0 / L[c * N + c];
        for (size_t i = c + 1; i < N; ++i) {
            double t = 0.0;
            for (size_t k = c; k < i; ++k) t -= L[i * N + k] * U[c * N + k];
            U[c * N + i] = t / L[i * N + i];
        }
    }
    out->assign(N * N, 0.0f);
    for (size_t i = 0; i < N; ++i) {
        for (size_t j = i; j < N; ++j) {
            double t = 0.0;
            for (size_t k = j; k < N; ++k) t += U[i * N + k] * U[j * N + k];
            const float v = static_cast<float>(t);
            (*out)[i * N + j] = v;
            (*out)[j * N + i] = v;
        }
    }
    return -1;
}

// not device_arrays_strict: nnz < 0 fails here (there it counts as no entries), num_rows is the caller's to check
bool device_arrays(const CSRMatrix* M) {
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

template <typename T>
bool copy_down(std::vector<T>* host, const T* device, size_t count, hipStream_t s) {
    host->resize(count);
    return count == 0 || hipMemcpyAsync(host->data(), device, count * sizeof(T), hipMemcpyDeviceToHost, s) == hipSuccess;
}

struct Builder {
    AMGHierarchy& H;
    AMGResult& res;
    hipStream_t stream;
    std::vector<float> diag{};    // diagonal_of's d of the level it ran on last

    int fail(SpMVError e, int level = -1, int row = -1) {
        res.error_code = code(e);
        res.bad_level = level;
        res.bad_row = row;
        return res.error_code;
    }

    // the level's structure (when asked for) and values on the host
    int download(int l, bool structure, std::vector<float>* va) {
        AMGLevel& lv = H.levels[static_cast<size_t>(l)];
        const CSRMatrix& M = lv.view;
        bool ok = copy_down(va, M.d_values, static_cast<size_t>(M.nnz), stream);
        if (structure) {
            ok = ok && copy_down(&lv.row_ptrs, M.d_row_ptrs, static_cast<size_t>(M.num_rows) + 1, stream) &&
                 copy_down(&lv.cols, M.d_col_indices, static_cast<size_t>(M.nnz), stream);
        }
        if (!ok || hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MEMCPY);
        }
        if (structure && l == 0 && !amg_structure_ok(M.num_rows, M.nnz, lv.row_ptrs.data(), lv.cols.data())) {
            return fail(SpMVError::INVALID_FORMAT);
        }
        return 0;
    }

    // the diagonal check and wd = omega / d on the device (d_wd allocated by the first call)
    int diagonal_of(int l, const std::vector<float>& va) {
        AMGLevel& lv = H.levels[static_cast<size_t>(l)];
        const int n = lv.view.num_rows;
        std::vector<float>& d = diag;
        std::vector<char> found;
        amg_diagonal(n, lv.row_ptrs.data(), lv.cols.data(), va.data(), &d, &found);
        std::vector<float> wd(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) {
            if (!found[i] || !(d[i] > 0.0f) || !std::isfinite(d[i])) return fail(SpMVError::INVALID_ARGUMENT, l, i);
            wd[i] = static_cast<float>(static_cast<double>(H.config.jacobi_weight) / static_cast<double>(d[i]));
        }
        if (!lv.d_wd && hipMalloc(reinterpret_cast<void**>(&lv.d_wd), static_cast<size_t>(n) * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MALLOC);
        }
        if (hipMemcpyAsync(lv.d_wd, wd.data(), wd.size() * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MEMCPY);
        }
        return 0;
    }

    // the coarsest level's solver: the dense inverse up to kAmgDenseRows rows, Jacobi sweeps above
    int coarse_solver(const std::vector<float>& va) {
        const int l = static_cast<int>(H.levels.size()) - 1;
        AMGLevel& lv = H.levels[static_cast<size_t>(l)];
        const int n = lv.view.num_rows;
        if (n > kAmgDenseRows) {
            H.coarse_solver = 1;
            return 0;
        }
        H.coarse_solver = 0;
        std::vector<float> inverse;
        const int bad = dense_inverse(n, lv.row_ptrs.data(), lv.cols.data(), va.data(), &inverse);
        if (bad >= 0) return fail(SpMVError::INVALID_ARGUMENT, l, bad);
        if (!H.d_cinv && hipMalloc(reinterpret_cast<void**>(&H.d_cinv), inverse.size() * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MALLOC);
        }
        if (hipMemcpyAsync(H.d_cinv, inverse.data(), inverse.size() * sizeof(float), hipMemcpyHostToDevice, stream) !=
                hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MEMCPY);
        }
        return 0;
    }

    // P, P^T, A P and A_{l+1} from the level's aggregate map; appends level l + 1
    int coarsen(int l, const std::vector<int>& agg, int count) {
        const int n = H.levels[static_cast<size_t>(l)].view.num_rows;
        CSRMatrix* P = csr_create(n, count, n);
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
            if (H.smoothed) {                                    // the unit P built below is the tentative one
                lv.T = P;
                lv.P = smoothed_P;
                lv.AT = AT;
            }
        }
        H.levels.emplace_back();
        H.levels.back().A = next;
        if (!P || !PT || !AP || !next || (H.smoothed && (!AT || !smoothed_P))) return fail(SpMVError::OUT_OF_MEMORY);
        for (int i = 0; i < n; ++i) {
            P->row_ptrs[i] = i;
            P->col_indices[i] = agg[static_cast<size_t>(i)];
            P->values[i] = 1.0f;
        }
        P->row_ptrs[n] = n;
        int status = csr_to_gpu(P);
        if (H.smoothed) {
            if (status == 0) status = smooth(l, false);
            if (status != 0) return fail(static_cast<SpMVError>(status));
            H.levels.back().view = device_view(next);
            return 0;
        }
        if (status == 0) status = csr_transpose_gpu(PT, P);
        if (status == 0) status = spgemm_csr(AP, &H.levels[static_cast<size_t>(l)].view, P);
        if (status == 0) status = spgemm_csr(next, PT, AP);
        if (status != 0) return fail(static_cast<SpMVError>(status));
        H.levels.back().view = device_view(next);
        return 0;
    }

    // the smoothed-aggregation step of level l with diagonal_of's d uploaded; an SpMVError code
    int smooth(int l, bool refill) {
        float* d_diag = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&d_diag), diag.size() * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return code(SpMVError::CUDA_MALLOC);
        }
        int status = 0;
        if (hipMemcpyAsync(d_diag, diag.data(), diag.size() * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            status = code(SpMVError::CUDA_MEMCPY);
        }
        if (status == 0) status = detail::amg_smooth_coarsen(H, l, d_diag, refill, stream);
        (void)hipFree(d_diag);
        return status;
    }

    int workspace(int l) {
        AMGLevel& lv = H.levels[static_cast<size_t>(l)];
        const size_t n = static_cast<size_t>(lv.view.num_rows);
        lv.lanes = detail::pick_lanes_per_row(static_cast<float>(lv.view.nnz) / static_cast<float>(n));
        if (hipMalloc(reinterpret_cast<void**>(&lv.d_work), (l == 0 ? 2 : 4) * n * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SpMVError::CUDA_MALLOC);
        }
        return 0;
    }

    void complexities() {
        double rows = 0.0, entries = 0.0;
        for (const AMGLevel& lv : H.levels) {
            rows += lv.view.num_rows;
            entries += lv.view.nnz;
        }
        res.levels = static_cast<int>(H.levels.size());
        res.coarse_solver = H.coarse_solver;
        res.grid_complexity = rows / H.num_rows;
        res.operator_complexity = H.nnz > 0 ? entries / H.nnz : 0.0;
    }
};

float ms_since(std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - start).count();
}

} // namespace

namespace detail {

bool amg_smoothing_ok(const AMGSmoothing& sm) {
    return sm.prolongator_weight > 0.0f && sm.prolongator_weight < 2.0f && sm.strength_decay > 0.0f &&
           sm.strength_decay <= 1.0f;
}

bool amg_config_ok(const AMGConfig& cfg) {
    return !(cfg.max_levels < 1 || cfg.coarse_rows < 1 || cfg.coarse_rows > kAmgDenseRows || !(cfg.strength >= 0.0f) ||
             cfg.pre_sweeps < 1 || cfg.post_sweeps < 0 || !(cfg.jacobi_weight > 0.0f && cfg.jacobi_weight < 2.0f) ||
             cfg.coarse_sweeps < 1);
}

int amg_level_workspace(AMGHierarchy& H, AMGResult& res, int l) {
    Builder b{H, res, nullptr};
    return b.workspace(l);
}

int amg_finish(AMGHierarchy& H, AMGResult& res, hipStream_t s) {
    Builder b{H, res, s};
    const int l = static_cast<int>(H.levels.size()) - 1;
    std::vector<float> va;
    if (H.levels[static_cast<size_t>(l)].view.num_rows <= kAmgDenseRows && b.download(l, true, &va) != 0) {
        return res.error_code;
    }
    if (b.coarse_solver(va) != 0) return res.error_code;
    b.complexities();
    return 0;
}

} // namespace detail

int amg_aggregate_cpu_csr(const CSRMatrix* A, float strength, int* aggregate_out, int* num_aggregates) {
    if (!A || !aggregate_out || !num_aggregates) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n < 0 || A->nnz < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values)) ||
        !amg_structure_ok(n, A->nnz, A->row_ptrs, A->col_indices)) {
        return code(SpMVError::INVALID_FORMAT);
    }
    if (!(strength >= 0.0f)) return code(SpMVError::INVALID_ARGUMENT);
    *num_aggregates = aggregate(n, A->row_ptrs, A->col_indices, A->values, strength, aggregate_out);
    return 0;
}

void amg_destroy(AMGHierarchy* H) {
    if (!H) return;
    for (AMGLevel& lv : H->levels) {
        if (lv.A) csr_destroy(lv.A);
        if (lv.P) csr_destroy(lv.P);
        if (lv.PT) csr_destroy(lv.PT);
        if (lv.AP) csr_destroy(lv.AP);
        if (lv.T) csr_destroy(lv.T);
        if (lv.AT) csr_destroy(lv.AT);
        if (lv.d_s) (void)hipFree(lv.d_s);
        if (lv.d_res) (void)hipFree(lv.d_res);
        if (lv.d_wd) (void)hipFree(lv.d_wd);
        if (lv.d_work) (void)hipFree(lv.d_work);
    }
    if (H->d_cinv) (void)hipFree(H->d_cinv);
    delete H;
}

namespace {

// amg_setup (smoothing == nullptr) and amg_setup_smoothed
AMGResult setup(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config, const AMGSmoothing* smoothing,
                const AMGAggregates* aggregates) {
    const auto start = std::chrono::steady_clock::now();
    AMGResult res;
    const auto fail = [&res](SpMVError e) {
        res.error_code = code(e);
        return res;
    };
    if (out) *out = nullptr;
    if (!out || !A) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols || A->num_rows < 1) return fail(SpMVError::INVALID_DIMENSION);
    if (!device_arrays(A)) return fail(SpMVError::INVALID_FORMAT);
    const AMGConfig defaults;
    const AMGConfig& cfg = config ? *config : defaults;
    if (!detail::amg_config_ok(cfg)) return fail(SpMVError::INVALID_ARGUMENT);
    if (smoothing && !detail::amg_smoothing_ok(*smoothing)) return fail(SpMVError::INVALID_ARGUMENT);
    // caller-given maps: sizes and contents, on the host
    int given = 0;
    std::vector<int> given_rows;        // n_{l+1} of each used map
    if (aggregates) {
        if (aggregates->levels < 0 || (aggregates->levels > 0 && !aggregates->map)) return fail(SpMVError::INVALID_ARGUMENT);
        for (int l = 0; l < aggregates->levels; ++l) {
            if (!aggregates->map[l]) return fail(SpMVError::INVALID_ARGUMENT);
        }
        given = std::min(aggregates->levels, cfg.max_levels - 1);
        int n = A->num_rows;
        for (int l = 0; l < given; ++l) {
            const int* map = aggregates->map[l];
            std::vector<char> used(static_cast<size_t>(n), 0);
            int top = -1;
            for (int i = 0; i < n; ++i) {
                if (map[i] < 0 || map[i] >= n) return fail(SpMVError::INVALID_ARGUMENT);
                used[static_cast<size_t>(map[i])] = 1;
                top = std::max(top, map[i]);
            }
            for (int a = 0; a <= top; ++a) {
                if (!used[static_cast<size_t>(a)]) return fail(SpMVError::INVALID_ARGUMENT);
            }
            n = top + 1;
            given_rows.push_back(n);
        }
    }

    const detail::TraceRange range(smoothing ? "spmv:amg_setup_smoothed" : "spmv:amg_setup");
    std::unique_ptr<AMGHierarchy, void (*)(AMGHierarchy*)> H(new AMGHierarchy, amg_destroy);
    H->config = cfg;
    if (smoothing) {
        H->smoothed = true;
        H->smoothing = *smoothing;
    }
    float theta = cfg.strength;      // theta_l: constant on a plain hierarchy
    H->num_rows = A->num_rows;
    H->nnz = A->nnz;
    H->levels.emplace_back();
    H->levels[0].view = device_view(A);
    Builder b{*H, res, detail::current_stream()};
    std::vector<float> va;
    for (int l = 0;; ++l) {
        if (b.download(l, true, &va) != 0 || b.diagonal_of(l, va) != 0 || b.workspace(l) != 0) return res;
        const AMGLevel& lv = H->levels[static_cast<size_t>(l)];
        const int n = lv.view.num_rows;
        std::vector<int> agg;
        int count = 0;
        if (aggregates) {
            if (l == given) break;
            agg.assign(aggregates->map[l], aggregates->map[l] + n);
            count = given_rows[static_cast<size_t>(l)];
        } else {
            if (n <= cfg.coarse_rows || l + 1 == cfg.max_levels) break;
            agg.resize(static_cast<size_t>(n));
            count = aggregate(n, lv.row_ptrs.data(), lv.cols.data(), va.data(), theta, agg.data());
            if (count == n) break;                      // nothing is strong any more
        }
        if (b.coarsen(l, agg, count) != 0) return res;
        if (smoothing) theta = theta * smoothing->strength_decay;
    }
    if (b.coarse_solver(va) != 0) return res;
    b.complexities();
    res.setup_ms = ms_since(start);
    *out = H.release();
    return res;
}

} // namespace

AMGResult amg_setup(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config, const AMGAggregates* aggregates) {
    return setup(out, A, config, nullptr, aggregates);
}

AMGResult amg_setup_smoothed(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config,
                             const AMGSmoothing* smoothing, const AMGAggregates* aggregates) {
    const AMGSmoothing defaults;
    return setup(out, A, config, smoothing ? smoothing : &defaults, aggregates);
}

int amg_is_smoothed(const AMGHierarchy* H) { return H && H->smoothed ? 1 : 0; }

int amg_level_transfer(const AMGHierarchy* H, int level, CSRMatrix* P_view, CSRMatrix* PT_view) {
    if (!H) return code(SpMVError::INVALID_ARGUMENT);
    if (level < 0 || level + 1 >= static_cast<int>(H->levels.size())) return code(SpMVError::INVALID_DIMENSION);
    const AMGLevel& lv = H->levels[static_cast<size_t>(level)];
    if (P_view) *P_view = device_view(lv.P);
    if (PT_view) *PT_view = device_view(lv.PT);
    return 0;
}

int amg_prolongator_cpu_csr(CSRMatrix* P, const CSRMatrix* A, const int* aggregate_map, int num_aggregates,
                            float weight) {
    if (!P || !A || !aggregate_map) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n < 0 || A->nnz < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values)) ||
        !amg_structure_ok(n, A->nnz, A->row_ptrs, A->col_indices)) {
        return code(SpMVError::INVALID_FORMAT);
    }
    if (!(weight > 0.0f && weight < 2.0f) || num_aggregates < 1) return code(SpMVError::INVALID_ARGUMENT);
    for (int i = 0; i < n; ++i) {
        if (aggregate_map[i] < 0 || aggregate_map[i] >= num_aggregates) return code(SpMVError::INVALID_ARGUMENT);
    }
    std::vector<float> d;
    std::vector<char> found;
    amg_diagonal(n, A->row_ptrs, A->col_indices, A->values, &d, &found);
    std::vector<float> scale(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        if (!found[i] || !(d[i] > 0.0f) || !std::isfinite(d[i])) return code(SpMVError::INVALID_ARGUMENT);
        scale[i] = static_cast<float>(-static_cast<double>(weight) / static_cast<double>(d[i]));
    }
    const std::unique_ptr<CSRMatrix, void (*)(CSRMatrix*)> T(csr_create(n, num_aggregates, n), csr_destroy),
        AT(csr_create(0, 0, 0), csr_destroy);
    if (!T || !AT) return code(SpMVError::OUT_OF_MEMORY);
    for (int i = 0; i < n; ++i) {
        T->row_ptrs[i] = i;
        T->col_indices[i] = aggregate_map[i];
        T->values[i] = 1.0f;
    }
    T->row_ptrs[n] = n;
    int status = spgemm_cpu_csr(AT.get(), A, T.get());
    if (status == 0) status = csr_scale_cpu(AT.get(), scale.data(), nullptr, AT->values);     // S, in place
    if (status == 0) status = csr_add_cpu(P, 1.0f, T.get(), 1.0f, AT.get());
    return status;
}

AMGResult amg_update(AMGHierarchy* H, const CSRMatrix* A) {
    const auto start = std::chrono::steady_clock::now();
    AMGResult res;
    const auto fail = [&res](SpMVError e) {
        res.error_code = code(e);
        return res;
    };
    if (!H || !A) return fail(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != H->num_rows || A->num_cols != H->num_rows || A->nnz != H->nnz) {
        return fail(SpMVError::INVALID_DIMENSION);
    }
    if (!device_arrays(A)) return fail(SpMVError::INVALID_FORMAT);
    if (H->device_built) return detail::amg_update_device(H, A);
    const detail::TraceRange range("spmv:amg_update");
    H->levels[0].view = device_view(A);
    Builder b{*H, res, detail::current_stream()};
    std::vector<float> va;
    const int levels = static_cast<int>(H->levels.size());
    for (int l = 0; l < levels; ++l) {
        if (b.download(l, l == 0, &va) != 0 || b.diagonal_of(l, va) != 0) return res;
        if (l + 1 == levels) break;
        AMGLevel& lv = H->levels[static_cast<size_t>(l)];
        int status = 0;
        if (H->smoothed) {
            status = b.smooth(l, true);
        } else {
            status = spgemm_csr_numeric(lv.AP, &lv.view, lv.P);
            if (status == 0) status = spgemm_csr_numeric(H->levels[static_cast<size_t>(l) + 1].A, lv.PT, lv.AP);
        }
        if (status != 0) return fail(static_cast<SpMVError>(status));
    }
    if (b.coarse_solver(va) != 0) return res;
    b.complexities();
    res.setup_ms = ms_since(start);
    return res;
}

int amg_num_levels(const AMGHierarchy* H) { return H ? static_cast<int>(H->levels.size()) : 0; }

int amg_setup_rounds(const AMGHierarchy* H, int level) {
    if (!H || level < 0 || level >= static_cast<int>(H->levels.size())) return 0;
    return H->levels[static_cast<size_t>(level)].rounds;
}

int amg_level(const AMGHierarchy* H, int level, CSRMatrix* view, const int** d_aggregate, int* num_aggregates) {
    if (!H) return code(SpMVError::INVALID_ARGUMENT);
    if (level < 0 || level >= static_cast<int>(H->levels.size())) return code(SpMVError::INVALID_DIMENSION);
    const AMGLevel& lv = H->levels[static_cast<size_t>(level)];
    if (view) *view = lv.view;
    const CSRMatrix* tentative = lv.T ? lv.T : lv.P;
    if (d_aggregate) *d_aggregate = tentative ? tentative->d_col_indices : nullptr;
    if (num_aggregates) *num_aggregates = lv.num_aggregates;
    return 0;
}

} // namespace spmv
