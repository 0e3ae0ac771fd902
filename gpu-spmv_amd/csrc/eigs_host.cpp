// eigs_host.cpp — the host side of include/spmv/eigs.h that needs no device: the host twin of sym_eig_small's
// Jacobi rule (the same operations as eigs.hip's one-workgroup kernel, each rounded separately: this file is compiled
// with -ffp-contract=off) and the argument checks of eigs_sym and sym_eig_small.
#include "eigs_impl.h"
#include "internal.h"

#include <cmath>
#include <cstdint>
#include <vector>

namespace spmv {
namespace detail {
namespace eigs {

void sym_eig_small_host(int n, const double* T, int ld, double* values, double* vectors) {
    std::vector<double> W(static_cast<size_t>(n) * n), S(static_cast<size_t>(n) * n, 0.0);
    double scale = 0.0;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            const double t = T[static_cast<size_t>(i) * ld + j];
            W[static_cast<size_t>(i) * n + j] = t;
            scale = std::fmax(scale, std::fabs(t));
        }
        S[static_cast<size_t>(i) * n + i] = 1.0;
    }
    const double thr = scale * 0x1p-53;
    const int N = (n + 1) & ~1;
    const int half = N / 2;
    int ps[kMaxOrder / 2], qs[kMaxOrder / 2];
    double cs[kMaxOrder / 2], sn[kMaxOrder / 2];
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool any = false;
        for (int r = 0; r < N - 1; ++r) {
            for (int k = 0; k < half; ++k) {
                int p, q;
                round_robin_pair(r, k, N, p, q);
                ps[k] = -1;
                if (q >= n) continue;
                const double apq = W[static_cast<size_t>(p) * n + q];
                if (!(std::fabs(apq) > thr)) continue;
                rotation(W[static_cast<size_t>(p) * n + p], W[static_cast<size_t>(q) * n + q], apq, cs[k], sn[k]);
                ps[k] = p;
                qs[k] = q;
                any = true;
            }
            for (int k = 0; k < half; ++k) {            // columns, of W and of S
                if (ps[k] < 0) continue;
                for (int i = 0; i < n; ++i) {
                    rotate_pair(cs[k], sn[k], W[static_cast<size_t>(i) * n + ps[k]], W[static_cast<size_t>(i) * n + qs[k]]);
                    rotate_pair(cs[k], sn[k], S[static_cast<size_t>(i) * n + ps[k]], S[static_cast<size_t>(i) * n + qs[k]]);
                }
            }
            for (int k = 0; k < half; ++k) {            // rows
                if (ps[k] < 0) continue;
                for (int j = 0; j < n; ++j) {
                    rotate_pair(cs[k], sn[k], W[static_cast<size_t>(ps[k]) * n + j], W[static_cast<size_t>(qs[k]) * n + j]);
                }
            }
            for (int k = 0; k < half; ++k) {
                if (ps[k] < 0) continue;
                W[static_cast<size_t>(ps[k]) * n + qs[k]] = 0.0;
                W[static_cast<size_t>(qs[k]) * n + ps[k]] = 0.0;
            }
        }
        if (!any) break;
    }
    for (int i = 0; i < n; ++i) {                       // rank by counting: ascending, ties by position
        const double di = W[static_cast<size_t>(i) * n + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double dj = W[static_cast<size_t>(j) * n + j];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        values[rank] = di;
        for (int l = 0; l < n; ++l) vectors[static_cast<size_t>(rank) * ld + l] = S[static_cast<size_t>(l) * n + i];
    }
}

int sym_eig_small_check(int n, const double* T, int ld, const double* values, const double* vectors,
                        bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!T || !values || !vectors || n < 0 || n > kMaxOrder || ld < n) return code(SpMVError::INVALID_ARGUMENT);
    *nothing_to_do = n == 0;
    return 0;
}

namespace {

bool overlap(const float* a, long long na, const float* b, long long nb) {
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) && b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

} // namespace

int eigs_check_arguments(const CSRMatrix* A, const float* d_values, const float* d_vectors, long long ldv,
                         const float* d_residuals, const float* d_v0, const EigsConfig& cfg, int* m,
                         bool* nothing_to_do) {
    *nothing_to_do = false;
    *m = 0;
    if (!A || !d_values || !d_vectors) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return 0;
    }
    if (!device_arrays_strict(A)) return code(SpMVError::INVALID_FORMAT);
    const int n = A->num_rows;
    const int k = cfg.num_values;
    if (k < 1 || k > kMaxValues || k > n) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.basis != 0 && (cfg.basis <= k || cfg.basis > kMaxOrder)) return code(SpMVError::INVALID_ARGUMENT);
    if (!(cfg.tolerance >= 0.0f)) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.max_iterations < 0) return code(SpMVError::INVALID_ARGUMENT);
    if ((cfg.which != EigsConfig::LARGEST && cfg.which != EigsConfig::SMALLEST) || cfg.engine < -1 || cfg.engine > 1) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    if (ldv < n) return code(SpMVError::INVALID_ARGUMENT);
    const long long span = static_cast<long long>(k - 1) * ldv + n;
    if (overlap(d_values, k, d_vectors, span) || overlap(d_values, k, d_residuals, k) ||
        overlap(d_residuals, k, d_vectors, span) || overlap(d_v0, n, d_vectors, span) ||
        overlap(d_v0, n, d_values, k) || overlap(d_v0, n, d_residuals, k)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const int wanted = cfg.basis != 0 ? cfg.basis : std::min(std::max(2 * k, 20), kMaxOrder);
    *m = std::min(wanted, n);
    return 0;
}

} // namespace eigs
} // namespace detail
} // namespace spmv
