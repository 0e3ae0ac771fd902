// ilu0.hip — kernels of the ILU(0) factorisation (include/spmv/ilu0.h).
//
// Row i of the factor needs the finished rows k < i of its own pattern: the dependency graph of a LOWER triangular
// solve, so the factorisation walks sptrsv_csr's LOWER level schedule with sptrsv.hip's two launch shapes (a grid over
// one wide level; one workgroup over a run of narrow levels with __syncthreads() in between, whose workgroup-scope
// release / acquire and the CU's write-through vector L1 make a level's stores the next level's plain loads).
//
// Inside a row, LANES lanes share the entries: entry t belongs to lane (t - begin) % LANES for the whole row, and only
// that lane ever loads or stores it, so no lane depends on another lane's store to row i.  The one value that crosses
// lanes, l_ik, is broadcast by a shuffle.  Every entry takes one operation per k in ascending k: the bits of
// ilu0_cpu_csr at every LANES.
//
// a and lu are deliberately not __restrict__ (they may be the same array, and lu is read and written in one launch);
// lu is never read through a const __restrict__ pointer, which would allow the scalar cache to serve it.
#include "internal.h"
#include "device_common.h"
#include "solver_common.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

// position of column `want` in cols[lo, hi) (strictly ascending), or -1
__device__ __forceinline__ int find_column(const int* __restrict__ cols, int lo, int hi, int want) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int c = cols[mid];
        if (c == want) return mid;
        if (c < want) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// Row pointers and column indices are clamped to the arrays, as in sptrsv_kernel: a matrix whose structure was
// rewritten behind the cached schedule gives wrong numbers, never an out-of-bounds access (and never an endless loop:
// the k loop advances one stored position per turn).
template <int LANES>
__global__ __launch_bounds__(kBlock)
void ilu0_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols, const float* a,
                 float* lu, const int* __restrict__ level_ptr, const int* __restrict__ order, int level_begin,
                 int level_end) {
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
            if (a != lu) {                           // the owner's first touch of its entries: A's values
                for (int t = begin + lane; t < end; t += LANES) lu[t] = a[t];
            }
            for (int pk = begin; pk < end; ++pk) {   // the same for every lane of the group
                const int k = cols[pk];
                if (k >= i || k < 0) break;          // columns ascend: the strict lower part is a prefix
                const int kb = max(row_ptrs[k], 0);
                const int ke = min(row_ptrs[k + 1], nnz);
                const int owner = (pk - begin) % LANES;
                float l = 0.0f;
                if (lane == owner) {
                    const int kd = find_column(cols, kb, ke, k);
                    l = __fdiv_rn(lu[pk], kd >= 0 ? lu[kd] : 0.0f);
                    lu[pk] = l;
                }
                if constexpr (LANES > 1) l = __shfl(l, owner, LANES);
                // this lane's entries right of pk (columns above k), each looked up in the finished row k
                int t = begin + lane;
                if (t <= pk) t += ((pk - t) / LANES + 1) * LANES;
                for (; t < end; t += LANES) {
                    const int q = find_column(cols, kb, ke, cols[t]);
                    if (q >= 0) lu[t] = __builtin_fmaf(-l, lu[q], lu[t]);
                }
            }
        }
        if (level + 1 < level_end) __syncthreads();
    }
}

// *out = min(*out, lowest row whose stored diagonal of lu is zero or not finite); one thread per row, after the
// factorisation in stream order.  An integer minimum: the same answer whatever the order.
__global__ __launch_bounds__(kBlock)
void ilu0_pivot_kernel(int n, int nnz, const int* __restrict__ row_ptrs, const int* __restrict__ cols,
                       const float* __restrict__ lu, unsigned* __restrict__ out) {
    unsigned worst = UINT_MAX;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int row = static_cast<int>(i);
        const int d = find_column(cols, max(row_ptrs[row], 0), min(row_ptrs[row + 1], nnz), row);
        const float u = d >= 0 ? lu[d] : 0.0f;
        if (!(u != 0.0f && isfinite(u))) worst = min(worst, static_cast<unsigned>(row));
    }
    for (int off = 32; off > 0; off >>= 1) worst = min(worst, __shfl_xor(worst, off, 64));
    if ((threadIdx.x & 63) == 0 && worst != UINT_MAX) atomicMin(out, worst);
}

template <int LANES>
hipError_t launch_groups(const SptrsvSchedule& sch, const CSRMatrix* A, const float* a, float* lu, hipStream_t s) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    for (const SptrsvSchedule::Group& g : sch.groups) {
        // a run of levels is one workgroup (the barrier is its only ordering); one level alone takes a grid
        const int grid = g.level_end - g.level_begin > 1 ? 1 : solver::grid_for_rows(g.rows, kRowsPerBlock);
        ilu0_kernel<LANES><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, a, lu,
                                                  sch.d_level_ptr, sch.d_order, g.level_begin, g.level_end);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace

hipError_t launch_ilu0(const SptrsvSchedule& schedule, const CSRMatrix* A, const float* d_a, float* d_lu,
                       int lanes_per_row, unsigned* d_zero_pivot, hipStream_t s) {
    const hipError_t e = solver::with_lanes(lanes_per_row, [&](auto L) {
        return launch_groups<decltype(L)::value>(schedule, A, d_a, d_lu, s);
    });
    if (e != hipSuccess || !d_zero_pivot) return e;
    ilu0_pivot_kernel<<<solver::vec_grid(A->num_rows), kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs,
                                                                       A->d_col_indices, d_lu, d_zero_pivot);
    return hipGetLastError();
}

} // namespace detail
} // namespace spmv
