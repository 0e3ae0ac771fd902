// bsr_diag_impl.h — what cg_bsr.hip (device) and bsr_diag_host.cpp (host twins, argument checks) share: the inverse of
// one diagonal block and the ordered apply of include/spmv/bsr.h written once, every fp64 and fp32 operation rounded
// separately on both sides.  Internal: not installed.
#ifndef SPMV_AMD_BSR_DIAG_IMPL_H
#define SPMV_AMD_BSR_DIAG_IMPL_H

#include "fsai_impl.h"
#include "spmv/bsr.h"
#include "spmv/cg.h"

#include <cmath>

#if defined(__HIPCC__)
#define BSR_DIAG_HD __host__ __device__ __forceinline__
#else
#define BSR_DIAG_HD inline
#endif

namespace spmv {
namespace detail {
namespace bsr {

using fsai::div_rn;
using fsai::sqrt_rn;
using fsai::tri;

// separately rounded products and sums: the device intrinsics; on the host the plain operators in a translation unit
// compiled with -ffp-contract=off (bsr_diag_host.cpp)
#if defined(__HIP_DEVICE_COMPILE__)
BSR_DIAG_HD double mul_rn(double a, double b) { return __dmul_rn(a, b); }
BSR_DIAG_HD double add_rn(double a, double b) { return __dadd_rn(a, b); }
BSR_DIAG_HD double sub_rn(double a, double b) { return __dsub_rn(a, b); }
BSR_DIAG_HD float mul_rn(float a, float b) { return __fmul_rn(a, b); }
BSR_DIAG_HD float add_rn(float a, float b) { return __fadd_rn(a, b); }
BSR_DIAG_HD bool finite(double a) { return isfinite(a); }
#else
BSR_DIAG_HD double mul_rn(double a, double b) { return a * b; }
BSR_DIAG_HD double add_rn(double a, double b) { return a + b; }
BSR_DIAG_HD double sub_rn(double a, double b) { return a - b; }
BSR_DIAG_HD float mul_rn(float a, float b) { return a * b; }
BSR_DIAG_HD float add_rn(float a, float b) { return a + b; }
BSR_DIAG_HD bool finite(double a) { return std::isfinite(a); }
#endif

// position of block column `want` in cols[lo, hi) (strictly ascending), or -1
BSR_DIAG_HD int find_block(const int* cols, int lo, int hi, int want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int c = cols[mid];
        if (c == want) return mid;
        if (c < want) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// The first two stages of diag_block_inverse, on the packed triangle T (fp64, every operation rounded on its own), for
// the callers that need the factor's inverse itself (bsr_tri_impl.h: block IC(0) stores fl32(L^-1)).  Rows and columns
// >= size are left as they are.
// Cholesky D = L L^T over T, row by row; false when a pivot w is not > 0 or not finite (the IEEE results are in T).
template <int B>
BSR_DIAG_HD bool packed_cholesky(double* T, int size) {
    bool ok = true;
#pragma unroll
    for (int p = 0; p < B; ++p) {
        if (p < size) {
#pragma unroll
            for (int q = 0; q <= p; ++q) {
                double w = T[tri(p, q)];
#pragma unroll
                for (int k = 0; k < q; ++k) w = sub_rn(w, mul_rn(T[tri(p, k)], T[tri(q, k)]));
                if (q == p) {
                    ok = ok && w > 0.0 && finite(w);
                    T[tri(p, p)] = sqrt_rn(w);
                } else {
                    T[tri(p, q)] = div_rn(w, T[tri(q, q)]);
                }
            }
        }
    }
    return ok;
}

// W = L^-1 over L, column j ascending: column j of L is last read when column j of W is written over it, and l_ii when
// column i is
template <int B>
BSR_DIAG_HD void packed_lower_inverse(double* T, int size) {
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (j < size) {
            T[tri(j, j)] = div_rn(1.0, T[tri(j, j)]);
#pragma unroll
            for (int i = j + 1; i < B; ++i) {
                if (i < size) {
                    double t = 0.0;
#pragma unroll
                    for (int k = j; k < i; ++k) t = add_rn(t, mul_rn(T[tri(i, k)], T[tri(k, j)]));
                    T[tri(i, j)] = div_rn(-t, T[tri(i, i)]);
                }
            }
        }
    }
}

// out (B * B floats, row-major) = fl32(D^-1) for the leading size x size part D of the stored block `block`, of which
// only the lower triangle is read; the other rows and columns of out are +0.0f.  1 <= size <= B.  In fp64:
//   Cholesky D = L L^T, row by row, w = d_pq - sum_{k<q} l_pk l_qk (k ascending), l_pp = sqrt(w), l_pq = w / l_qq
//   W = L^-1 column by column: w_jj = 1 / l_jj, w_ij = -(sum_{k=j..i-1} l_ik w_kj) / l_ii (k ascending, from +0)
//   D^-1_ij = sum_{k >= max(i,j)} w_ki w_kj (k ascending, from +0), computed for i >= j and mirrored
// all in one packed triangle T.  false, with out unspecified, when a pivot w is not > 0 or not finite.
template <int B>
BSR_DIAG_HD bool diag_block_inverse(const float* block, int size, float* out) {
    double T[B * (B + 1) / 2];
#pragma unroll
    for (int p = 0; p < B; ++p) {
#pragma unroll
        for (int q = 0; q <= p; ++q) T[tri(p, q)] = p < size ? static_cast<double>(block[p * B + q]) : 0.0;
    }
    if (!packed_cholesky<B>(T, size)) return false;
    packed_lower_inverse<B>(T, size);
#pragma unroll
    for (int i = 0; i < B; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = i; k < B; ++k) {
                if (k < size) s = add_rn(s, mul_rn(T[tri(k, i)], T[tri(k, j)]));
            }
            const float v = i < size ? static_cast<float>(s) : 0.0f;
            out[i * B + j] = v;
            out[j * B + i] = v;
        }
    }
    return true;
}

// z_i for scalar row i = I * B + k of an n-row matrix: the ordered sum of include/spmv/bsr.h (bsr_diag_apply_cpu);
// inv_row is row k of block I's inverse, r_block the B entries of r that start at I * B (read below n only)
template <int B>
BSR_DIAG_HD float diag_apply_row(const float* inv_row, const float* r_block, long long first, int n) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < B; ++c) {
        if (first + c < n) s = add_rn(s, mul_rn(inv_row[c], r_block[c]));
    }
    return s;
}

// the argument checks of the device entry points, which need no device (bsr_diag_host.cpp)
int diag_check(const BSRMatrix* A, const void* out, bool device);
// cg_solve_bsr's checks before the device, in cg_solve's order; *nothing_to_do: no rows, SUCCESS and converged
int cg_check(const BSRMatrix* A, const float* d_b, const float* d_x, const CGConfig& cfg, bool* nothing_to_do);

} // namespace bsr
} // namespace detail
} // namespace spmv

#endif
