// bsr_tri.hip — the kernels of block IC(0) and of the block triangular solve (include/spmv/bsr_factor.h, DESIGN.md
// §4.31).  Both walk a level schedule of the BLOCK pattern through the level layer of device_common.h
// (for_each_level_row, launch_level_groups), which also says why a level's plain loads see the previous level's stores.
//
// A group of LANES lanes (1 .. 64, inside one wavefront) owns a block row.
//
// The factorisation.  The ownership unit is one row r of one block: unit u = (t - begin) * B + r of block row I, owned
// by lane u % LANES for the whole block row.  ONLY THE OWNER of a unit loads or stores its elements in f during the
// launch level that makes block row I (factor0.hip's rule), so no lane depends on another lane's store to block row I.
// What crosses lanes crosses in registers: the finished L_IK (B * B floats) is broadcast by shuffles from the owners of
// its rows, and W_II's lower triangle is gathered the same way for the fp64 stage, which every lane of the group then
// runs on its own copy (the lanes move in lockstep: the copies cost nothing) so that each owner stores its own row of
// V_I.  No LDS.  The mirror of L_IK, to (K,I), is stored by the owner of the row and never read in the launch level that
// writes it: block row I's updates take L_IK from the registers, and (K,I) is read only by block rows below I, which
// store (I', I) left of their diagonal and so lie on a later level.
// Every element takes the operations of bsr_ic0_cpu in its order (K ascending, then m ascending): the same bits at
// every LANES.
//
// a, f, b and x are deliberately not __restrict__ (a and f, b and x may be the same array; f and x are read and written
// in one launch), and f is never read through a const __restrict__ pointer, which would allow the scalar cache to
// serve it.
//
// Block row pointers, block columns and the schedule's entries are clamped to the arrays: a structure rewritten behind
// a cached schedule gives wrong numbers, never an out-of-range access (every block position that is loaded or stored
// lies in [max(brp[R], 0), min(brp[R + 1], num_blocks)) of some block row R in [0, block_rows), every x index below n)
// and never an endless loop (the K loop advances one stored position per turn).
#include "bsr_device.h"
#include "bsr_tri_impl.h"
#include "device_common.h"
#include "internal.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace spmv {
namespace detail {
namespace bsr {

namespace {

using namespace dev;

// row `r` (run-time) of a B x B block held in registers, by selects: no dynamic register index
template <int B>
__device__ __forceinline__ void select_row(const float (&M)[B * B], int r, float (&row)[B]) {
#pragma unroll
    for (int c = 0; c < B; ++c) row[c] = M[c];
#pragma unroll
    for (int rr = 1; rr < B; ++rr) {
#pragma unroll
        for (int c = 0; c < B; ++c) row[c] = rr == r ? M[rr * B + c] : row[c];
    }
}

template <int B, int LANES>
__global__ __launch_bounds__(kBlock)
void bsr_ic0_kernel(int n, int block_rows, int num_blocks, const int* __restrict__ brp, const int* __restrict__ bc,
                    const float* a, float* f, const int* __restrict__ level_ptr, const int* __restrict__ order,
                    int level_begin, int level_end, unsigned* pivot) {
    constexpr int BB = B * B;
    for_each_level_row<LANES>(level_ptr, order, level_begin, level_end, block_rows,
                              [=](bool live, auto row, int lane) {
        if (!live) return;
        const int I = row();
        const int begin = max(brp[I], 0);
        const int end = min(brp[I + 1], num_blocks);
        const int di = find_block(bc, begin, end, I);
        if (di < 0) return;
        const int size = min(B, n - I * B);      // scalar rows of this block row inside the matrix
        const int units = (di - begin + 1) * B;  // rows of the blocks on and left of the diagonal
        if (a != f) {                            // the owner's first touch of its rows: A's values
            for (int u = lane; u < units; u += LANES) {
                const long long at = static_cast<long long>(begin + u / B) * BB + (u % B) * B;
#pragma unroll
                for (int c = 0; c < B; ++c) f[at + c] = a[at + c];
            }
        }
        for (int pk = begin; pk < di; ++pk) {
            const int K = bc[pk];
            if (K >= I || K < 0) break;          // block columns ascend: the strict lower part is a prefix
            const int kb = max(brp[K], 0);
            const int ke = min(brp[K + 1], num_blocks);
            const int kd = find_block(bc, kb, ke, K);
            const int mirror = find_block(bc, kb, ke, I);          // (K,I): L^T for the rows below and the solves
            const int u0 = (pk - begin) * B;     // unit of row 0 of block pk
            float V[BB];                         // the finished block (K,K); only m <= c of row c is used
#pragma unroll
            for (int c = 0; c < B; ++c) {
#pragma unroll
                for (int m = 0; m < B; ++m) {
                    V[c * B + m] = (m <= c && kd >= 0) ? f[static_cast<long long>(kd) * BB + c * B + m] : 0.0f;
                }
            }
            // step 1: the owners of block pk's rows finish them, store them and their mirror
            float L[BB];
#pragma unroll
            for (int r = 0; r < B; ++r) {
                float l[B];
#pragma unroll
                for (int c = 0; c < B; ++c) l[c] = 0.0f;
                if ((u0 + r) % LANES == lane) {
                    const long long at = static_cast<long long>(pk) * BB + r * B;
                    if (r < size) {
                        float w[B];
#pragma unroll
                        for (int c = 0; c < B; ++c) w[c] = f[at + c];
                        ic_scale_row<B>(w, V, l);
                    }
#pragma unroll
                    for (int c = 0; c < B; ++c) f[at + c] = l[c];
                    if (mirror >= 0) {
#pragma unroll
                        for (int c = 0; c < B; ++c) f[static_cast<long long>(mirror) * BB + c * B + r] = l[c];
                    }
                }
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    if constexpr (LANES > 1) L[r * B + c] = __shfl(l[c], (u0 + r) % LANES, LANES);
                    else L[r * B + c] = l[c];
                }
            }
            // steps 2 and 3: this lane's rows right of block pk
            int u = lane;
            if (u < u0 + B) u += ((u0 + B - 1 - u) / LANES + 1) * LANES;
            for (; u < units; u += LANES) {
                const int t = begin + u / B;
                const int r = u % B;
                if (r >= size) continue;
                float l[B];
                select_row<B>(L, r, l);
                const long long at = static_cast<long long>(t) * BB + r * B;
                if (t == di) {
                    float w[B];
#pragma unroll
                    for (int c = 0; c < B; ++c) w[c] = f[at + c];
                    ic_diag_row<B>(l, L, r, w);
#pragma unroll
                    for (int c = 0; c < B; ++c) f[at + c] = w[c];
                    continue;
                }
                const int q = find_block(bc, kb, ke, bc[t]);
                if (q < 0) continue;
                float Fq[BB], w[B];
#pragma unroll
                for (int e = 0; e < BB; ++e) Fq[e] = f[static_cast<long long>(q) * BB + e];
#pragma unroll
                for (int c = 0; c < B; ++c) w[c] = f[at + c];
                ic_update_row<B>(l, Fq, w);
#pragma unroll
                for (int c = 0; c < B; ++c) f[at + c] = w[c];
            }
        }
        // the diagonal stage: gather W_II's lower triangle from the owners of its rows, fp64 on every lane's copy
        const int ud = (di - begin) * B;
        double T[B * (B + 1) / 2];
#pragma unroll
        for (int r = 0; r < B; ++r) {
            const bool mine = (ud + r) % LANES == lane;
#pragma unroll
            for (int c = 0; c <= r; ++c) {
                float w = 0.0f;
                if (mine && r < size) w = f[static_cast<long long>(di) * BB + r * B + c];
                if constexpr (LANES > 1) w = __shfl(w, (ud + r) % LANES, LANES);
                T[tri(r, c)] = static_cast<double>(w);
            }
        }
        const bool ok = ic_diag_stage<B>(T, size);
#pragma unroll
        for (int r = 0; r < B; ++r) {
            if ((ud + r) % LANES == lane) {
#pragma unroll
                for (int c = 0; c < B; ++c) {
                    f[static_cast<long long>(di) * BB + r * B + c] = ic_v_entry<B>(T, r, c, size);
                }
            }
        }
        if (!ok && lane == 0 && pivot) atomicMin(pivot, static_cast<unsigned>(I));
    });
}

// ORDERED (LANES == 1): sptrsv_cpu_bsr's order and roundings.  Otherwise bsr_device.h's walk over the triangle's blocks
// with fused multiply-adds and group_sum's fixed butterfly; lane 0 applies the diagonal step by the ordered rule.
template <int B, int LANES, bool WIDE, bool ORDERED>
__global__ __launch_bounds__(kBlock)
void bsr_sptrsv_kernel(int n, int block_rows, int num_blocks, const int* __restrict__ brp,
                       const int* __restrict__ bc, const float* __restrict__ bv, const float* b, float* x,
                       const int* __restrict__ level_ptr, const int* __restrict__ order, int level_begin,
                       int level_end, int upper, int unit) {
    static_assert(!ORDERED || LANES == 1, "the ordered solve is one lane per block row");
    constexpr int BB = B * B;
    for_each_level_row<LANES>(level_ptr, order, level_begin, level_end, block_rows,
                              [=](bool live, auto row, int lane) {
        int I = 0, begin = 0, end = 0;
        float acc[B];
#pragma unroll
        for (int r = 0; r < B; ++r) acc[r] = 0.0f;
        if (live) {
            I = row();
            begin = max(brp[I], 0);
            end = min(brp[I + 1], num_blocks);
            // the triangle's side of I; a block column at or past block_rows would start at or past n
            block_row_partial_dot<B, LANES, WIDE, true, ORDERED>(bc, bv, x, n, begin, end, lane,
                                                                 upper ? I + 1 : 0, upper ? block_rows : I, acc);
        }
        if constexpr (LANES > 1) {
#pragma unroll
            for (int r = 0; r < B; ++r) acc[r] = group_sum<LANES>(acc[r]);
        }
        if (live && lane == 0) {
            const int size = min(B, n - I * B);
            float t[B];
#pragma unroll
            for (int r = 0; r < B; ++r) t[r] = r < size ? __fsub_rn(b[I * B + r], acc[r]) : 0.0f;
            if (!unit) {
                const int d = find_block(bc, begin, end, I);
                float V[BB];
#pragma unroll
                for (int e = 0; e < BB; ++e) V[e] = d >= 0 ? bv[static_cast<long long>(d) * BB + e] : 0.0f;
                float u[B];
#pragma unroll
                for (int r = 0; r < B; ++r) u[r] = tri_diag_row<B>(V, t, r, size, upper != 0);
#pragma unroll
                for (int r = 0; r < B; ++r) t[r] = u[r];
            }
#pragma unroll
            for (int r = 0; r < B; ++r) {
                if (r < size) x[I * B + r] = t[r];
            }
        }
    });
}

// one thread per scalar row: the diagonal entry (k,k) of the stored block (I,I) of F must be > 0 and finite
template <int B>
__global__ __launch_bounds__(kBlock)
void bsr_factor_diag_check_kernel(const int* __restrict__ brp, const int* __restrict__ bc,
                                  const float* __restrict__ bv, int n, int block_rows, int num_blocks,
                                  int* __restrict__ flag) {
    bool bad = false;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int I = static_cast<int>(i / B), k = static_cast<int>(i % B);
        const int at = find_block(bc, max(brp[I], 0), min(brp[I + 1], num_blocks), I);
        const float d = at >= 0 ? bv[(static_cast<long long>(at) * B + k) * B + k] : 0.0f;
        bad = bad || !(at >= 0 && d > 0.0f && isfinite(d));
    }
    if (bad) *flag = 1;
}

template <int B, int LANES>
hipError_t launch_ic0_groups(const SptrsvSchedule& sch, const BSRMatrix* A, const float* a, float* f, unsigned* pivot,
                             hipStream_t s) {
    return launch_level_groups<LANES>(sch, [&](int grid, int level_begin, int level_end) {
        bsr_ic0_kernel<B, LANES><<<grid, kBlock, 0, s>>>(A->num_rows, A->num_block_rows, A->num_blocks,
                                                         A->d_block_row_ptrs, A->d_block_cols, a, f, sch.d_level_ptr,
                                                         sch.d_order, level_begin, level_end, pivot);
    });
}

template <int B, int LANES, bool WIDE, bool ORDERED>
hipError_t launch_solve_groups(const SptrsvSchedule& sch, const BSRMatrix* F, const float* b, float* x, int upper,
                               int unit, hipStream_t s) {
    return launch_level_groups<LANES>(sch, [&](int grid, int level_begin, int level_end) {
        bsr_sptrsv_kernel<B, LANES, WIDE, ORDERED><<<grid, kBlock, 0, s>>>(
            F->num_rows, F->num_block_rows, F->num_blocks, F->d_block_row_ptrs, F->d_block_cols, F->d_values, b, x,
            sch.d_level_ptr, sch.d_order, level_begin, level_end, upper, unit);
    });
}

} // namespace

hipError_t launch_bsr_ic0(const SptrsvSchedule& schedule, const BSRMatrix* A, const float* d_a, float* d_f, int lanes,
                          unsigned* d_pivot, hipStream_t s) {
    return with_block_dim(A->block_dim, [&](auto Bc) {
        return with_lanes(lanes, [&](auto L) {
            return launch_ic0_groups<decltype(Bc)::value, decltype(L)::value>(schedule, A, d_a, d_f, d_pivot, s);
        });
    });
}

hipError_t launch_sptrsv_bsr(const SptrsvSchedule& schedule, const BSRMatrix* F, const float* d_b, float* d_x, int uplo,
                             int unit_diagonal, bool ordered, int lanes, hipStream_t s) {
    const bool wide = aligned16(F->d_values);
    return with_block_dim(F->block_dim, [&](auto Bc) {
        constexpr int B = decltype(Bc)::value;
        constexpr bool kCanWide = B * B % 4 == 0;
        if (ordered) {
            if (kCanWide && wide) {
                return launch_solve_groups<B, 1, kCanWide, true>(schedule, F, d_b, d_x, uplo, unit_diagonal, s);
            }
            return launch_solve_groups<B, 1, false, true>(schedule, F, d_b, d_x, uplo, unit_diagonal, s);
        }
        return with_lanes(lanes, [&](auto L) {
            constexpr int LANES = decltype(L)::value;
            if (kCanWide && wide) {
                return launch_solve_groups<B, LANES, kCanWide, false>(schedule, F, d_b, d_x, uplo, unit_diagonal, s);
            }
            return launch_solve_groups<B, LANES, false, false>(schedule, F, d_b, d_x, uplo, unit_diagonal, s);
        });
    });
}

hipError_t launch_factor_diag_check(const BSRMatrix* F, int* flag, hipStream_t s) {
    return with_block_dim(F->block_dim, [&](auto Bc) {
        bsr_factor_diag_check_kernel<decltype(Bc)::value><<<vec_grid(F->num_rows), kBlock, 0, s>>>(
            F->d_block_row_ptrs, F->d_block_cols, F->d_values, F->num_rows, F->num_block_rows, F->num_blocks, flag);
        return hipGetLastError();
    });
}

} // namespace bsr
} // namespace detail
} // namespace spmv
