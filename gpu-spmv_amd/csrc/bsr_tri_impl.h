// bsr_tri_impl.h — what bsr_tri.hip (device), bsr_tri_host.cpp (host twins, checks, drivers) and cg_bsr.hip (the solver
// on the factor) share: the row arithmetic of block IC(0) and of the block triangular solve of include/spmv/bsr_factor.h
// written once, and the launch layer between the drivers and the kernels.  Internal: not installed.
#ifndef SPMV_AMD_BSR_TRI_IMPL_H
#define SPMV_AMD_BSR_TRI_IMPL_H

#include "bsr_diag_impl.h"
#include "internal.h"
#include "spmv/bsr_factor.h"

#include <memory>

namespace spmv {
namespace detail {
namespace bsr {

// ---- block IC(0): one row r of one block at a time (the ownership unit of the kernel) ----
// step 1: row r of L_IK = W_IK L_KK^-T.  w: row r of W_IK; V: the stored block (K,K), of which row c's entries m <= c
// are read
template <int B>
BSR_DIAG_HD void ic_scale_row(const float* w, const float* V, float* l) {
#pragma unroll
    for (int c = 0; c < B; ++c) {
        float s = 0.0f;
#pragma unroll
        for (int m = 0; m <= c; ++m) s = __builtin_fmaf(w[m], V[c * B + m], s);
        l[c] = s;
    }
}

// step 2: row r of W_IJ -= L_IK L_JK^T.  l: row r of L_IK; Fq: the stored block (K,J), which holds L_JK^T
template <int B>
BSR_DIAG_HD void ic_update_row(const float* l, const float* Fq, float* w) {
#pragma unroll
    for (int c = 0; c < B; ++c) {
        float s = w[c];
#pragma unroll
        for (int m = 0; m < B; ++m) s = __builtin_fmaf(-l[m], Fq[m * B + c], s);
        w[c] = s;
    }
}

// step 3: row r of the diagonal block, its entries c <= r.  l: row r of L_IK; L: all of L_IK
template <int B>
BSR_DIAG_HD void ic_diag_row(const float* l, const float* L, int r, float* w) {
#pragma unroll
    for (int c = 0; c < B; ++c) {
        float s = w[c];
#pragma unroll
        for (int m = 0; m < B; ++m) s = __builtin_fmaf(-l[m], L[c * B + m], s);
        w[c] = c <= r ? s : w[c];
    }
}

// the diagonal stage on the packed fp64 triangle T of W_II (rows >= size hold 0.0 and stay): T = L_II^-1.  false when
// a pivot was not > 0 or not finite; the IEEE results are in T either way
template <int B>
BSR_DIAG_HD bool ic_diag_stage(double* T, int size) {
    const bool ok = packed_cholesky<B>(T, size);
    packed_lower_inverse<B>(T, size);
    return ok;
}

// entry (r, c) of the stored block V_I from the finished triangle
template <int B>
BSR_DIAG_HD float ic_v_entry(const double* T, int r, int c, int size) {
    const int hi = r > c ? r : c, lo = r > c ? c : r;
    return hi < size ? static_cast<float>(T[tri(hi, lo)]) : 0.0f;
}

// ---- block triangular solve: the diagonal step of one block row.  V: the stored block (I,I); t: b - s, B entries ----
template <int B>
BSR_DIAG_HD float tri_diag_row(const float* V, const float* t, int r, int size, bool upper) {
    float u = 0.0f;
#pragma unroll
    for (int c = 0; c < B; ++c) {
        const bool take = upper ? (c >= r && c < size) : c <= r;
        if (take) u = add_rn(u, mul_rn(V[r * B + c], t[c]));
    }
    return u;
}

// ---- the launch layer (bsr_tri.hip) and the drivers' shared front (bsr_tri_host.cpp) ----
// the `uplo` schedule of M's block pattern: a CSR header over the block structure arrays handed to sptrsv_schedule_for,
// so the side table entry under d_block_row_ptrs serves every matrix over those arrays
int tri_schedule_for(const BSRMatrix* M, int uplo, hipStream_t stream, ScheduleRef* out, float* analysis_ms);
// lanes per block row: spmv_bsr's rule on the triangle's mean blocks per block row (SPMV_DEBUG=bsr_tri_lanes=N)
int tri_lanes(const SptrsvSchedule& schedule, bool ordered);
// cg_solve_bsr_ic's checks 2 - 4 on F (after cg_check on A)
int cg_ic_check(const BSRMatrix* A, const BSRMatrix* F);

hipError_t launch_sptrsv_bsr(const SptrsvSchedule& schedule, const BSRMatrix* F, const float* d_b, float* d_x, int uplo,
                             int unit_diagonal, bool ordered, int lanes, hipStream_t s);
// d_pivot (may be null): preset to all ones; the lowest block row with a bad pivot is folded in by an unsigned minimum
hipError_t launch_bsr_ic0(const SptrsvSchedule& schedule, const BSRMatrix* A, const float* d_a, float* d_f, int lanes,
                          unsigned* d_pivot, hipStream_t s);
// *flag = 1 when a diagonal block of F is missing or holds a diagonal entry that is not > 0 or not finite
hipError_t launch_factor_diag_check(const BSRMatrix* F, int* flag, hipStream_t s);

} // namespace bsr
} // namespace detail
} // namespace spmv

#endif
