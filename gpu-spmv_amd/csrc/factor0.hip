// factor0.hip — the kernels of the two zero-fill factorisations: ILU(0) (include/spmv/ilu0.h) and
// IC(0) (include/spmv/ic0.h).  One kernel template over (KIND, LANES); what IC(0) does differently is
// an `if constexpr (KIND == IC0)` branch inside it.
//
// Row i of the factor needs the finished rows k < i of its own pattern: the dependency graph of a LOWER triangular
// solve, so the factorisation walks sptrsv_csr's LOWER level schedule, launched by the level layer of device_common.h
// (launch_level_groups).  The walk is for_each_level_row's, written out (through the helper ilu0_csr measured 0.8 %
// slower on a 4 M-row matrix with every resource equal: profiles/level_layer_ab.txt); the helper's comment says why a
// level's plain loads see the previous level's stores.
//
// Inside a row, LANES lanes share the entries (IC: those on and left of the diagonal): entry t belongs to lane
// (t - begin) % LANES for the whole row, and only that lane ever loads or stores it, so no lane depends on another
// lane's store to row i.  The one value that crosses lanes, l_ik, is broadcast by a shuffle.  Every entry takes one
// operation per k in ascending k: the bits of ilu0_cpu_csr / ic0_cpu_csr at every LANES.
//
// IC only.  The update of w_ij needs l_jk, an entry of row j, not of row k; the factor keeps L^T in the upper
// positions, so l_jk is read from position (k,j) of the finished row k, by the same "look the column up in row k"
// search as ILU(0).  That position was stored by the owner of l_jk in row j, which mirrors each l_jk to (k,j) as soon
// as it has divided: j is stored in row i left of the diagonal, so level(j) < level(i), and the store happened in an
// earlier launch or before an earlier barrier of this workgroup.  The mirror of l_ik itself, to (k,i), is never read
// in the launch level that makes it: the diagonal update takes l_ik from the register.
//
// a and f are deliberately not __restrict__ (they may be the same array, and f is read and written in one launch);
// f is never read through a const __restrict__ pointer, which would allow the scalar cache to serve it.
//
// Row pointers and column indices are clamped to the arrays, as in sptrsv_kernel: a matrix whose structure was
// rewritten behind the cached schedule gives wrong numbers, never an out-of-bounds access (every position that is
// loaded or stored lies in [max(row_ptrs[r], 0), min(row_ptrs[r + 1], nnz)) of some row r in [0, n)) and never an
// endless loop (the k loop advances one stored position per turn).
#include "internal.h"
#include "device_common.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

template <Factor0Kind KIND, int LANES>
__global__ __launch_bounds__(kBlock)
void factor0_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols, const float* a,
                    float* f, const int* __restrict__ level_ptr, const int* __restrict__ order, int level_begin,
                    int level_end) {
    constexpr bool kIC = KIND == Factor0Kind::IC0;
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    for (int level = level_begin; level < level_end; ++level) {
        const int first = level_ptr[level];
        const int last = min(level_ptr[level + 1], n);
        for (long long base = first + static_cast<long long>(blockIdx.x) * kRowsPerBlock; base < last;
             base += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
            const long long r = base + slot;
            if (r < 0 || r >= last) continue;        // the whole LANES group leaves together: no shuffle reads it
            const int i = min(max(order[r], 0), n - 1);
            const int begin = max(row_ptrs[i], 0);
            const int end = min(row_ptrs[i + 1], nnz);
            int di = end;                            // IC: the diagonal's position, the same for every lane of the group
            if constexpr (kIC) {
                di = find_column(cols, begin, end, i);
                if (di < 0) continue;
            }
            // ILU factors the whole row and IC stops at the diagonal: [begin, stop) are the row's entries, and the
            // k loop looks for the strict lower part in [begin, lower_end)
            const int stop = kIC ? di + 1 : end;
            const int lower_end = kIC ? di : end;
            if (a != f) {                            // the owner's first touch of its entries: A's values
                for (int t = begin + lane; t < stop; t += LANES) f[t] = a[t];
            }
            for (int pk = begin; pk < lower_end; ++pk) {
                const int k = cols[pk];
                if (k >= i || k < 0) break;          // columns ascend: the strict lower part is a prefix
                const int kb = max(row_ptrs[k], 0);
                const int ke = min(row_ptrs[k + 1], nnz);
                const int owner = (pk - begin) % LANES;
                float lik = 0.0f;
                if (lane == owner) {
                    const int kd = find_column(cols, kb, ke, k);
                    lik = __fdiv_rn(f[pk], kd >= 0 ? f[kd] : 0.0f);
                    f[pk] = lik;
                    if constexpr (kIC) {
                        const int mirror = find_column(cols, kb, ke, i);     // (k,i): L^T for the rows below and the solves
                        if (mirror >= 0) f[mirror] = lik;
                    }
                }
                if constexpr (LANES > 1) lik = __shfl(lik, owner, LANES);
                // this lane's entries right of pk, each looked up in the finished row k (IC: (k,j) holds l_jk)
                int t = begin + lane;
                if (t <= pk) t += ((pk - t) / LANES + 1) * LANES;
                for (; t < stop; t += LANES) {
                    if constexpr (kIC) {
                        if (t == di) {
                            f[t] = __builtin_fmaf(-lik, lik, f[t]);
                            continue;
                        }
                    }
                    const int q = find_column(cols, kb, ke, cols[t]);
                    if (q >= 0) f[t] = __builtin_fmaf(-lik, f[q], f[t]);
                }
            }
            if constexpr (kIC) {
                // the correctly rounded IEEE square root (the compiler's default for fp32; not the native approximation)
                if (lane == (di - begin) % LANES) f[di] = __builtin_sqrtf(f[di]);
            }
        }
        if (level + 1 < level_end) __syncthreads();
    }
}

// *out = min(*out, lowest row whose stored diagonal of f is a bad pivot: zero (ILU) or not > 0 (IC), or not finite);
// one thread per row, after the factorisation in stream order.  An integer minimum: the same answer whatever the order.
template <Factor0Kind KIND>
__global__ __launch_bounds__(kBlock)
void factor0_pivot_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                          const float* __restrict__ f, unsigned* __restrict__ out) {
    unsigned worst = UINT_MAX;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int row = static_cast<int>(i);
        const int d = find_column(cols, max(row_ptrs[row], 0), min(row_ptrs[row + 1], nnz), row);
        const float u = d >= 0 ? f[d] : 0.0f;
        bool usable;
        if constexpr (KIND == Factor0Kind::IC0) usable = u > 0.0f;
        else usable = u != 0.0f;
        if (!(usable && isfinite(u))) worst = min(worst, static_cast<unsigned>(row));
    }
    for (int off = 32; off > 0; off >>= 1) worst = min(worst, __shfl_xor(worst, off, 64));
    if ((threadIdx.x & 63) == 0 && worst != UINT_MAX) atomicMin(out, worst);
}

template <Factor0Kind KIND, int LANES>
hipError_t launch_groups(const SptrsvSchedule& sch, const CSRMatrix* A, const float* a, float* f, hipStream_t s) {
    return launch_level_groups<LANES>(sch, [&](int grid, int level_begin, int level_end) {
        factor0_kernel<KIND, LANES><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, a, f,
                                                            sch.d_level_ptr, sch.d_order, level_begin, level_end);
    });
}

template <Factor0Kind KIND>
hipError_t launch_kind(const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_a, float* d_out,
                       int lanes_per_row, unsigned* d_pivot, hipStream_t s) {
    const hipError_t e = with_lanes(lanes_per_row, [&](auto L) {
        return launch_groups<KIND, decltype(L)::value>(schedule, A, d_a, d_out, s);
    });
    if (e != hipSuccess || !d_pivot) return e;
    factor0_pivot_kernel<KIND><<<vec_grid(A->num_rows), kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                        A->d_col_indices, d_out, d_pivot);
    return hipGetLastError();
}

} // namespace

hipError_t launch_factor0(Factor0Kind kind, const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_a,
                          float* d_out, int lanes_per_row, unsigned* d_pivot, hipStream_t s) {
    if (kind == Factor0Kind::IC0) return launch_kind<Factor0Kind::IC0>(schedule, A, d_a, d_out, lanes_per_row, d_pivot, s);
    return launch_kind<Factor0Kind::ILU0>(schedule, A, d_a, d_out, lanes_per_row, d_pivot, s);
}

} // namespace detail
} // namespace spmv
