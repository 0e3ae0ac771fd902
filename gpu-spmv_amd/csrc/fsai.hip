// fsai.hip — the kernels of the factorised sparse approximate inverse (include/spmv/fsai.h).
//
// Structure pass, O(nnz_A + nnz_S), one thread per row:
//   fsai_count_kernel     validates a row of A and of S and counts the entries of S's row on or left of the diagonal.
//                         The findings go to five info words by integer atomics (or, min, max): the same words
//                         whatever the arrival order.  A row whose pointers are malformed is flagged and not walked.
//   (transpose.hip's exclusive scan turns the counts into G's row pointers)
//   fsai_columns_kernel   copies the columns j <= i of S's row i into G.
//
// Numeric kernel, the hot path: one group of LANES lanes per row of G, a whole number of groups per wavefront, rows
// independent of each other.  A group keeps in LDS its pattern P (m ints), the packed lower triangle T (m(m+1)/2
// doubles) that holds M = A[P,P] first and C in the end, and u (m doubles).  CLASS is the capacity of the slab: the
// groups per wavefront follow from it (a wavefront's slabs stay inside kWaveLds bytes where one fits at all), and
// lanes of a wavefront beyond its last group idle.
//   gather          lane p walks the lower part of row j_p of A in a two-pointer merge against P and writes M_p.;
//                   absent entries stay +0.0
//   Cholesky        column by column: the lanes share the entries (p,q), p >= q, each doing its k loop alone and
//                   leaving w in place; the owner of (q,q) takes the root; after a wavefront-level synchronisation the
//                   lanes below it divide
//   substitution    q descending, one u_q published per step; u_p is its own accumulator until lane p % LANES, the
//                   only lane that ever writes it, finishes it
// Every entry takes fsai_impl.h's operation sequence, the one fsai_cpu_csr takes: the same bits at every LANES and
// CLASS.  The groups of a wavefront have different m: every loop that holds a synchronisation runs to the wavefront's
// largest m with the lanes of shorter rows doing nothing, and no lane leaves before the last one.
//
// Row pointers, columns and m are clamped to the arrays and to CLASS, as in factor0_kernel: fsai_csr_numeric does not
// validate again, and a structure rewritten behind it gives wrong numbers, never an access outside the arrays or LDS.
// No float atomics, no waiting between workgroups.
#include "internal.h"
#include "device_common.h"
#include "fsai_impl.h"

#include <hip/hip_runtime.h>

#include <climits>

namespace spmv {
namespace detail {
namespace fsai {

namespace {

using namespace dev;

// LDS stores of this wavefront before, its LDS loads after (assemble.hip's rule)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one row of a CSR structure: malformed (pointers or a column), not strictly ascending, entries with column <= i,
// (i,i) stored.  A row with malformed pointers is not walked.
struct RowFindings {
    bool bad_format = false, unsorted = false, diagonal = false;
    int lower = 0;
};

__device__ __forceinline__ RowFindings check_row(const int* __restrict__ rp, const int* __restrict__ cols, int n,
                                                 int nnz, int i) {
    RowFindings f;
    const int b = rp[i], e = rp[i + 1];
    if (b < 0 || e > nnz || b > e) {
        f.bad_format = true;
        return f;
    }
    int previous = -1;
    for (int t = b; t < e; ++t) {
        const int c = cols[t];
        if (c < 0 || c >= n) f.bad_format = true;
        if (t > b && c <= previous) f.unsorted = true;
        previous = c;
        if (c <= i) ++f.lower;
        if (c == i) f.diagonal = true;
    }
    return f;
}

__global__ __launch_bounds__(kBlock)
void fsai_count_kernel(int n, int a_nnz, const int* __restrict__ a_rp, const int* __restrict__ a_cols, int s_nnz,
                       const int* __restrict__ s_rp, const int* __restrict__ s_cols, int* __restrict__ counts,
                       unsigned* __restrict__ info) {
    const bool same = a_rp == s_rp && a_cols == s_cols && a_nnz == s_nnz;
    bool bad = false, unsorted = false, no_diagonal = false;
    unsigned long_row = UINT_MAX;
    int longest = 0;
    for (long long r = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; r <= n;
         r += static_cast<long long>(gridDim.x) * kBlock) {
        const int i = static_cast<int>(r);
        if (i == n) {
            counts[n] = 0;
            continue;
        }
        const RowFindings fs = check_row(s_rp, s_cols, n, s_nnz, i);
        bad = bad || fs.bad_format;
        unsorted = unsorted || fs.unsorted;
        if (!same) {
            const RowFindings fa = check_row(a_rp, a_cols, n, a_nnz, i);
            bad = bad || fa.bad_format;
            unsorted = unsorted || fa.unsorted;
        }
        if (!fs.bad_format && !fs.diagonal) no_diagonal = true;
        if (fs.lower > kFsaiMaxRow) long_row = min(long_row, static_cast<unsigned>(i));
        longest = max(longest, fs.lower);
        counts[i] = fs.lower;
    }
    // every lane is back here: one atomic per wavefront and word
    for (int off = 32; off > 0; off >>= 1) {
        long_row = min(long_row, static_cast<unsigned>(__shfl_xor(static_cast<int>(long_row), off, 64)));
        longest = max(longest, __shfl_xor(longest, off, 64));
    }
    const bool any_bad = __ballot(bad) != 0, any_unsorted = __ballot(unsorted) != 0;
    const bool any_no_diagonal = __ballot(no_diagonal) != 0;
    if ((threadIdx.x & 63) != 0) return;
    if (any_bad) atomicOr(&info[kBadFormat], 1u);
    if (any_unsorted) atomicOr(&info[kUnsorted], 1u);
    if (any_no_diagonal) atomicOr(&info[kNoDiagonal], 1u);
    if (long_row != UINT_MAX) atomicMin(&info[kLongRow], long_row);
    if (longest > 0) atomicMax(&info[kMaxRow], static_cast<unsigned>(longest));
}

// S validated: its row i is walked once more and the columns j <= i go to G's row
__global__ __launch_bounds__(kBlock)
void fsai_columns_kernel(int n, const int* __restrict__ s_rp, const int* __restrict__ s_cols,
                         const int* __restrict__ g_rp, int* __restrict__ g_cols) {
    for (long long r = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; r < n;
         r += static_cast<long long>(gridDim.x) * kBlock) {
        const int i = static_cast<int>(r);
        int o = g_rp[i];
        const int o_end = g_rp[i + 1];
        for (int t = s_rp[i]; t < s_rp[i + 1] && o < o_end; ++t) {
            const int c = s_cols[t];
            if (c <= i) g_cols[o++] = c;
        }
    }
}

// ---- the numeric kernel ----
constexpr int kWaveLds = 12288;       // bytes of slabs per wavefront where more than one group fits

template <int CLASS>
struct Slab {
    static constexpr int kTri = CLASS * (CLASS + 1) / 2;
    static constexpr int kBytes = kTri * 8 + CLASS * 8 + CLASS * 4;
    // class 64: three wavefronts of one 17 KiB slab each stay inside 64 KiB of LDS
    static constexpr int kWaves = CLASS == 64 ? 3 : 4;
    static constexpr int kFit = kWaveLds / kBytes > 1 ? kWaveLds / kBytes : 1;
};

template <int CLASS, int LANES>
constexpr int groups_per_wave() {
    return 64 / LANES < Slab<CLASS>::kFit ? 64 / LANES : Slab<CLASS>::kFit;
}

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int CLASS, int LANES>
__global__ __launch_bounds__(Slab<CLASS>::kWaves * 64)
void fsai_numeric_kernel(int n, int a_nnz, const int* __restrict__ a_rp, const int* __restrict__ a_cols,
                         const float* __restrict__ a_vals, int g_nnz, const int* __restrict__ g_rp,
                         const int* __restrict__ g_cols, float* __restrict__ g_vals) {
    constexpr int kGroupsPerWave = groups_per_wave<CLASS, LANES>();
    constexpr int kGroups = kGroupsPerWave * Slab<CLASS>::kWaves;       // rows per workgroup and trip
    constexpr int kTri = Slab<CLASS>::kTri;
    __shared__ double s_tri[kGroups * kTri];
    __shared__ double s_u[kGroups * CLASS];
    __shared__ int s_pattern[kGroups * CLASS];

    const int wave = threadIdx.x >> 6;
    const int group = (threadIdx.x & 63) / LANES;
    const int lane = threadIdx.x % LANES;
    const bool has_slab = group < kGroupsPerWave;
    const int slot = wave * kGroupsPerWave + (has_slab ? group : 0);
    double* T = s_tri + slot * kTri;
    double* U = s_u + slot * CLASS;
    int* P = s_pattern + slot * CLASS;

    for (long long base = static_cast<long long>(blockIdx.x) * kGroups; base < n;
         base += static_cast<long long>(gridDim.x) * kGroups) {
        const long long row = base + wave * kGroupsPerWave + group;
        int gb = 0, m = 0;
        if (has_slab && row < n) {
            gb = clamped(g_rp[row], 0, g_nnz);
            m = clamped(clamped(g_rp[row + 1], 0, g_nnz) - gb, 0, CLASS);
        }
        int wave_m = m;                  // the wavefront's longest row bounds every loop with a synchronisation in it
        for (int off = 32; off > 0; off >>= 1) wave_m = max(wave_m, __shfl_xor(wave_m, off, 64));

        for (int p = lane; p < m; p += LANES) {
            P[p] = clamped(g_cols[gb + p], 0, n - 1);
            U[p] = 0.0;
        }
        for (int t = lane; t < tri(m, 0); t += LANES) T[t] = 0.0;
        wave_sync();

        // gather: row j_p of A against P[0 .. p]; both ascend
        for (int p = lane; p < m; p += LANES) {
            const int j = P[p];
            const int ab = clamped(a_rp[j], 0, a_nnz);
            const int ae = clamped(a_rp[j + 1], 0, a_nnz);
            int q = 0;
            for (int t = ab; t < ae; ++t) {
                const int c = a_cols[t];
                if (c > j) break;
                while (q <= p && P[q] < c) ++q;
                if (q > p) break;
                if (P[q] == c) T[tri(p, q)] = static_cast<double>(a_vals[t]);
            }
        }
        wave_sync();

        // Cholesky C C^T = M in place
        for (int q = 0; q < wave_m; ++q) {
            for (int p = q + lane; p < m; p += LANES) {
                const double w = cholesky_w(T, p, q);
                T[tri(p, q)] = p == q ? sqrt_rn(w) : w;
            }
            wave_sync();
            if (q < m) {
                const double cqq = T[tri(q, q)];
                for (int p = q + lane; p < m; p += LANES) {
                    if (p > q) T[tri(p, q)] = div_rn(T[tri(p, q)], cqq);
                }
            }
            wave_sync();
        }

        // u = C^-T e_m
        for (int q = wave_m - 1; q >= 0; --q) {
            if (q < m && lane == q % LANES) U[q] = substitution_u(U[q], T[tri(q, q)], q == m - 1);
            wave_sync();
            if (q < m) {
                const double uq = U[q];
                for (int p = lane; p < q; p += LANES) U[p] = substitution_t(T[tri(q, p)], uq, U[p]);
            }
        }

        for (int p = lane; p < m; p += LANES) g_vals[gb + p] = static_cast<float>(U[p]);     // its own u_p
        wave_sync();                     // the next trip rewrites the slab
    }
}

// *out = min(*out, lowest row whose last stored entry, g_ii, is not > 0 or not finite); factor0_pivot_kernel's rule
__global__ __launch_bounds__(kBlock)
void fsai_bad_row_kernel(int n, int g_nnz, const int* __restrict__ g_rp, const float* __restrict__ g_vals,
                         unsigned* __restrict__ out) {
    unsigned worst = UINT_MAX;
    for (long long r = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; r < n;
         r += static_cast<long long>(gridDim.x) * kBlock) {
        const int b = clamped(g_rp[r], 0, g_nnz);
        const int e = clamped(g_rp[r + 1], 0, g_nnz);
        const float d = e > b ? g_vals[e - 1] : 0.0f;
        if (!(d > 0.0f && isfinite(d))) worst = min(worst, static_cast<unsigned>(r));
    }
    for (int off = 32; off > 0; off >>= 1) worst = min(worst, __shfl_xor(worst, off, 64));
    if ((threadIdx.x & 63) == 0 && worst != UINT_MAX) atomicMin(out, worst);
}

template <int CLASS>
hipError_t launch_class(const CSRMatrix* A, int n, int g_nnz, const int* g_rp, const int* g_cols, float* g_vals,
                        int lanes, hipStream_t s) {
    return with_lanes(lanes, [&](auto L) {
        constexpr int LANES = decltype(L)::value;
        constexpr int kRowsPerBlock = groups_per_wave<CLASS, LANES>() * Slab<CLASS>::kWaves;
        fsai_numeric_kernel<CLASS, LANES><<<capped_grid(n, kRowsPerBlock), Slab<CLASS>::kWaves * 64, 0, s>>>(
            n, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, g_nnz, g_rp, g_cols, g_vals);
        return hipGetLastError();
    });
}

} // namespace

hipError_t launch_structure_count(const CSRMatrix* A, const CSRMatrix* S, int* counts, unsigned* info, hipStream_t s) {
    const int n = A->num_rows;
    fsai_count_kernel<<<vec_grid(static_cast<long long>(n) + 1), kBlock, 0, s>>>(
        n, A->nnz, A->d_row_ptrs, A->d_col_indices, S->nnz, S->d_row_ptrs, S->d_col_indices, counts, info);
    return hipGetLastError();
}

hipError_t launch_structure_columns(const CSRMatrix* S, const int* g_row_ptrs, int* g_cols, hipStream_t s) {
    fsai_columns_kernel<<<vec_grid(S->num_rows), kBlock, 0, s>>>(S->num_rows, S->d_row_ptrs, S->d_col_indices,
                                                                 g_row_ptrs, g_cols);
    return hipGetLastError();
}

hipError_t launch_numeric(const CSRMatrix* A, int n, int g_nnz, const int* g_row_ptrs, const int* g_cols,
                          float* g_values, int row_class, int lanes, unsigned* bad_row, hipStream_t s) {
    hipError_t e;
    switch (row_class) {
        case 4:  e = launch_class<4>(A, n, g_nnz, g_row_ptrs, g_cols, g_values, lanes, s); break;
        case 8:  e = launch_class<8>(A, n, g_nnz, g_row_ptrs, g_cols, g_values, lanes, s); break;
        case 16: e = launch_class<16>(A, n, g_nnz, g_row_ptrs, g_cols, g_values, lanes, s); break;
        case 32: e = launch_class<32>(A, n, g_nnz, g_row_ptrs, g_cols, g_values, lanes, s); break;
        default: e = launch_class<64>(A, n, g_nnz, g_row_ptrs, g_cols, g_values, lanes, s); break;
    }
    if (e != hipSuccess || !bad_row) return e;
    fsai_bad_row_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, g_nnz, g_row_ptrs, g_values, bad_row);
    return hipGetLastError();
}

} // namespace fsai
} // namespace detail
} // namespace spmv
