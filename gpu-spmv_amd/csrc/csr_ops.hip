// csr_ops.hip — CSR algebra on the device (include/spmv/csr_ops.h): C = alpha*A + beta*B and its
// values-only refill, bit for bit csr_add_cpu's result at every lane count; row / column scaling; the diagonal in and
// out.  No sort, no hash table, no atomics, no LDS, no workgroup waits for another.
//
// The sum is ONE kernel in three modes.  A group of LANES lanes owns a row; its lanes stride over the row of A in
// tiles of LANES, then over the row of B.
//   COUNT    checks both rows (bounds of the row pointers before anything follows them, then every column in [0, n)
//            and above its left neighbour), looks every entry of A up in B's row and stores
//            len(A) + len(B) - matches; an exclusive scan turns the counts into C's row pointers.
//   WRITE    merge by rank.  Entry i_a of A with column c goes to slot i_a + lower_bound_B(c) - (matched entries of A
//            before i_a): the last term is a popcount of the group's part of a __ballot of the match flags, below the
//            lane, plus a carry from the tiles before.  It writes fl(alpha a), or fl(fl(alpha a) + fl(beta b)) when B
//            holds c.  An unmatched entry j_b of B goes to j_b + lower_bound_A(c) - (matched entries of B before
//            j_b) and writes fl(beta b); a matched one writes nothing.  One writer per slot, and neither the slot nor
//            the value depends on LANES.
//   REFILL   COUNT's checks and WRITE's slots, with every slot compared with C's column instead of written and the
//            row's count compared with C's row length: csr_add_numeric, one launch.
// A row of more than kLongTiles tiles of its group (A and B together) is left to the whole wavefront, which takes
// the long rows of its groups one after another at 64 lanes once the groups are through the others: a hub row does
// not hold a narrow group for thousands of tiles.  Neither slots nor values depend on the path.
// The searches gallop from where the lane's previous search ended (the columns ascend, so the bounds do too): a lane
// that walks a long row alone pays for the gaps, not for log2 of the row at every entry.
#include "csr_ops_impl.h"
#include "internal.h"
#include "device_common.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace spmv {
namespace detail {
namespace csr_ops {

namespace {

using dev::capped_grid;
using dev::kBlock;
using dev::vec_grid;

constexpr int kWaves = kBlock / 64;
constexpr int kLongTiles = 32;            // a row of more tiles than this goes to a whole wavefront

enum Mode { COUNT = 0, WRITE = 1, REFILL = 2 };

struct MatView {
    const int* rp;
    const int* ci;
    const float* va;
    long long nnz;
};

struct AddArgs {
    MatView A, B;
    int m, n;
    float alpha, beta;
    int* counts;              // COUNT: [m + 1], counts[m] = 0
    long long* partial;       // COUNT: per wavefront of the grid {entries of C, common columns, longest row}
    const int* c_rp;          // WRITE, REFILL
    int* c_ci;                // WRITE: written; REFILL: compared
    float* c_va;
    long long c_nnz;          // REFILL
    int* flag;                // COUNT, REFILL: a check failed
};

// first p in [lo, hi) with cols[p] >= want, hi when there is none; everything left of lo is known to be below `want`.
// Gallops from lo, then bisects.  Never reads outside [lo, hi), whatever the array holds.
__device__ __forceinline__ int lower_bound_from(const int* __restrict__ cols, int lo, int hi, int want) {
    int top = lo, step = 1;
    while (top < hi && cols[top] < want) {
        lo = top + 1;
        top = hi - top > step ? top + step : hi;
        step <<= 1;
    }
    hi = min(top, hi);
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cols[mid] < want) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the bits of this lane's group in a wavefront ballot
template <int LANES>
__device__ __forceinline__ unsigned long long group_bits(unsigned long long ballot) {
    if constexpr (LANES == 64) {
        return ballot;
    } else {
        return (ballot >> ((threadIdx.x & 63) / LANES * LANES)) & ((1ull << LANES) - 1ull);
    }
}

// row `row` of a matrix whose row pointers nobody has checked: false unless 0 <= begin <= end <= nnz, the first row
// begins at 0 and the last ends at nnz (over all rows: rp[0] == 0, no decrease, rp[m] == nnz)
__device__ __forceinline__ bool row_bounds(const int* __restrict__ rp, long long row, int m, long long nnz,
                                           int* begin, int* end) {
    const int lo = rp[row], hi = rp[row + 1];
    *begin = lo;
    *end = hi;
    bool ok = lo >= 0 && lo <= hi && hi <= nnz;
    if (row == 0 && lo != 0) ok = false;
    if (row == m - 1 && hi != nnz) ok = false;
    return ok;
}

// One row, walked by a group of LANES lanes (lane = this thread's place in it); the bounds are checked or zero.
// sum_nnz, sum_common and top are the COUNT totals of the calling thread.
template <int LANES, int MODE>
__device__ __forceinline__ void add_row(const AddArgs& g, long long row, int lane, int a0, int a1, int b0, int b1,
                                        int c0, int c1, bool& bad, long long& sum_nnz, long long& sum_common,
                                        long long& top) {
    const unsigned long long below = (1ull << lane) - 1ull;
    const MatView& A = g.A;
    const MatView& B = g.B;
    const int la = a1 - a0, lb = b1 - b0, lc = c1 - c0;

    // ---- the row of A ----
    int matched = 0;                         // matched entries in the tiles before this one
    int hint = b0;
    for (int t0 = 0; t0 < la; t0 += LANES) {
        const int ia = t0 + lane;
        const bool active = ia < la;
        bool match = false;
        int col = 0;
        if (active) {
            col = A.ci[a0 + ia];
            if (MODE != WRITE && (col < 0 || col >= g.n || (ia > 0 && col <= A.ci[a0 + ia - 1]))) bad = true;
            hint = lower_bound_from(B.ci, hint, b1, col);
            match = hint < b1 && B.ci[hint] == col;
        }
        const unsigned long long bits = group_bits<LANES>(__ballot(match));
        if (MODE != COUNT && active) {
            const int out = ia + (hint - b0) - (matched + __popcll(bits & below));
            float v = __fmul_rn(g.alpha, A.va[a0 + ia]);
            if (match) v = __fadd_rn(v, __fmul_rn(g.beta, B.va[hint]));
            if (MODE == WRITE) {
                g.c_ci[c0 + out] = col;
                g.c_va[c0 + out] = v;
            } else if (out >= 0 && out < lc && g.c_ci[c0 + out] == col) {
                g.c_va[c0 + out] = v;
            } else {
                bad = true;
            }
        }
        matched += __popcll(bits);
    }
    const long long count = static_cast<long long>(la) + lb - matched;

    // ---- the row of B ----
    if (MODE == COUNT) {
        for (int jb = lane; jb < lb; jb += LANES) {
            const int col = B.ci[b0 + jb];
            if (col < 0 || col >= g.n || (jb > 0 && col <= B.ci[b0 + jb - 1])) bad = true;
        }
    } else {
        int matched_b = 0;
        hint = a0;
        for (int t0 = 0; t0 < lb; t0 += LANES) {
            const int jb = t0 + lane;
            const bool active = jb < lb;
            bool match = false;
            int col = 0;
            if (active) {
                col = B.ci[b0 + jb];
                if (MODE != WRITE && (col < 0 || col >= g.n || (jb > 0 && col <= B.ci[b0 + jb - 1]))) bad = true;
                hint = lower_bound_from(A.ci, hint, a1, col);
                match = hint < a1 && A.ci[hint] == col;
            }
            const unsigned long long bits = group_bits<LANES>(__ballot(match));
            if (active && !match) {
                const int out = jb + (hint - a0) - (matched_b + __popcll(bits & below));
                const float v = __fmul_rn(g.beta, B.va[b0 + jb]);
                if (MODE == WRITE) {
                    g.c_ci[c0 + out] = col;
                    g.c_va[c0 + out] = v;
                } else if (out >= 0 && out < lc && g.c_ci[c0 + out] == col) {
                    g.c_va[c0 + out] = v;
                } else {
                    bad = true;
                }
            }
            matched_b += __popcll(bits);
        }
    }

    if (MODE == COUNT && row < g.m && lane == 0) {
        const int clamped = count > INT_MAX ? INT_MAX : static_cast<int>(count);
        g.counts[row] = clamped;
        sum_nnz += count;
        sum_common += matched;
        top = max(top, static_cast<long long>(clamped));
    }
    if (MODE == REFILL && row < g.m && count != lc) bad = true;
}

// A group of LANES lanes per row.  A row with more than kLongTiles tiles of LANES entries in A and B together is not
// walked by its group: once the groups of the wavefront are through their rows of the trip, the whole wavefront takes
// the long ones, one after another, 64 lanes wide.  Which path a row takes changes neither its slots nor its values.
template <int LANES, int MODE>
__global__ __launch_bounds__(kBlock) void csr_add_kernel(AddArgs g) {
    constexpr int kRowsPerBlock = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    bool bad = false;
    long long sum_nnz = 0, sum_common = 0, top = 0;
    if (MODE == COUNT && blockIdx.x == 0 && threadIdx.x == 0) g.counts[g.m] = 0;

    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < g.m;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long row = first + slot;
        int a0 = 0, a1 = 0, b0 = 0, b1 = 0, c0 = 0, c1 = 0;
        if (row < g.m) {
            if (MODE == WRITE) {
                a0 = g.A.rp[row];
                a1 = g.A.rp[row + 1];
                b0 = g.B.rp[row];
                b1 = g.B.rp[row + 1];
                c0 = g.c_rp[row];
            } else {
                bool ok = row_bounds(g.A.rp, row, g.m, g.A.nnz, &a0, &a1);
                ok = row_bounds(g.B.rp, row, g.m, g.B.nnz, &b0, &b1) && ok;
                if (MODE == REFILL) ok = row_bounds(g.c_rp, row, g.m, g.c_nnz, &c0, &c1) && ok;
                if (!ok) {                       // nothing of this row is followed
                    bad = true;
                    a0 = a1 = b0 = b1 = c0 = c1 = 0;
                }
            }
        }
        const bool is_long = LANES < 64 && static_cast<long long>(a1 - a0) + (b1 - b0) > kLongTiles * LANES;
        if (!is_long) add_row<LANES, MODE>(g, row, lane, a0, a1, b0, b1, c0, c1, bad, sum_nnz, sum_common, top);
        if constexpr (LANES < 64) {
            // (every lane of the wavefront is here: the trip count depends on the workgroup alone)
            unsigned long long pending = __ballot(is_long && lane == 0);
            while (pending) {
                const int src = __ffsll(static_cast<long long>(pending)) - 1;
                pending &= pending - 1;
                add_row<64, MODE>(g, first + (threadIdx.x & ~63) / LANES + src / LANES, threadIdx.x & 63,
                                  __shfl(a0, src, 64), __shfl(a1, src, 64), __shfl(b0, src, 64), __shfl(b1, src, 64),
                                  __shfl(c0, src, 64), __shfl(c1, src, 64), bad, sum_nnz, sum_common, top);
            }
        }
    }

    if (MODE == COUNT) {
        for (int off = 32; off > 0; off >>= 1) {
            sum_nnz += __shfl_xor(sum_nnz, off, 64);
            sum_common += __shfl_xor(sum_common, off, 64);
            top = max(top, __shfl_xor(top, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            long long* mine = g.partial + 3 * (static_cast<long long>(blockIdx.x) * kWaves + (threadIdx.x >> 6));
            mine[0] = sum_nnz;
            mine[1] = sum_common;
            mine[2] = top;
        }
    }
    if (MODE != WRITE) {
        if (__any(bad) && (threadIdx.x & 63) == 0) *g.flag = 1;     // (every writer stores the same 1)
    }
}

// out[p] = a[p] * (r[row of p] * c[col of p]), each product rounded; the row by upper_bound only where r is given
__global__ __launch_bounds__(kBlock) void csr_scale_kernel(const int* __restrict__ rp, const int* __restrict__ ci,
                                                           const float* va, int rows, long long nnz,
                                                           const float* __restrict__ r, const float* __restrict__ c,
                                                           float* out) {
    for (long long p = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; p < nnz;
         p += static_cast<long long>(gridDim.x) * kBlock) {
        float v = va[p];
        if (r) {
            const float ri = r[dev::upper_bound(rp, 0, rows + 1, p) - 1];
            v = c ? __fmul_rn(v, __fmul_rn(ri, c[ci[p]])) : __fmul_rn(v, ri);
        } else if (c) {
            v = __fmul_rn(v, c[ci[p]]);
        }
        out[p] = v;
    }
}

// diag[i] = 0.0f + the stored (i, i) entries of row i in storage order (solver_common.h diag_kernel's sum)
__global__ __launch_bounds__(kBlock) void csr_diagonal_kernel(int rows, const int* __restrict__ rp,
                                                              const int* __restrict__ ci,
                                                              const float* __restrict__ va, float* __restrict__ diag) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < rows;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        float d = 0.0f;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (ci[p] == i) d = __fadd_rn(d, va[p]);
        }
        diag[i] = d;
    }
}

__global__ __launch_bounds__(kBlock) void csr_diag_matrix_kernel(int n, const float* __restrict__ diag,
                                                                 int* __restrict__ rp, int* __restrict__ ci,
                                                                 float* __restrict__ va) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i <= n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        rp[i] = static_cast<int>(i);
        if (i < n) {
            ci[i] = static_cast<int>(i);
            va[i] = diag ? diag[i] : 1.0f;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
MatView view_of(const CSRMatrix* M) { return MatView{M->d_row_ptrs, M->d_col_indices, M->d_values, M->nnz}; }

// lanes per row from the mean of the two rows' lengths together
int add_lanes_for(const CSRMatrix* A, const CSRMatrix* B) {
    if (int f = forced_lanes("add_lanes")) return f;
    const float both = static_cast<float>(A->nnz) + static_cast<float>(B->nnz);
    return pick_lanes_per_row(both / static_cast<float>(std::max(A->num_rows, 1)));
}

template <int MODE>
hipError_t launch_add(int lanes, int grid, const AddArgs& args, hipStream_t s) {
    return dev::with_lanes(lanes, [&](auto L) {
        csr_add_kernel<decltype(L)::value, MODE><<<grid, kBlock, 0, s>>>(args);
        return hipGetLastError();
    });
}

int add_build(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B, CsrAddResult* result,
              hipStream_t s) {
    *result = CsrAddResult();
    const int status = add_check(C, A, B, false);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    const TraceRange range("spmv:csr_add");
    const int m = A->num_rows, n = A->num_cols;
    const int lanes = add_lanes_for(A, B);
    const int grid = capped_grid(m, kBlock / lanes);
    result->lanes = lanes;

    // ---- counting pass and scan; the counts become C's row pointers only after the checks passed ----
    const std::vector<long long> levels = device_scan_levels(static_cast<long long>(m) + 1);
    const size_t waves = static_cast<size_t>(grid) * kWaves;
    DevBuf<int> counts, scan_sums, flag;
    DevBuf<long long> partial;
    if (dev_alloc(&counts, static_cast<long long>(m) + 1) != hipSuccess ||
        dev_alloc(&scan_sums, device_scan_sums(levels)) != hipSuccess || dev_alloc(&flag, 1) != hipSuccess ||
        dev_alloc(&partial, 3LL * static_cast<long long>(waves)) != hipSuccess) {
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    Events ev;
    AddArgs args{};
    args.A = view_of(A);
    args.B = view_of(B);
    args.m = m;
    args.n = n;
    args.alpha = alpha;
    args.beta = beta;
    args.counts = counts.get();
    args.partial = partial.get();
    args.flag = flag.get();
    std::vector<long long> host_partial(3 * waves);
    int bad = 0;
    bool ok = ev.ok && hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
              hipEventRecord(ev.e[0], s) == hipSuccess && launch_add<COUNT>(lanes, grid, args, s) == hipSuccess &&
              device_exclusive_scan(counts.get(), levels, scan_sums.get(), s) == hipSuccess &&
              hipEventRecord(ev.e[1], s) == hipSuccess &&
              hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess &&
              hipMemcpyAsync(host_partial.data(), partial.get(), host_partial.size() * sizeof(long long),
                             hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    result->launches = 1 + device_scan_launches(levels);
    if (bad) return fail(result, SpMVError::INVALID_FORMAT);
    long long nnz = 0, common = 0, longest = 0;
    for (size_t w = 0; w < waves; ++w) {
        nnz += host_partial[3 * w];
        common += host_partial[3 * w + 1];
        longest = std::max(longest, host_partial[3 * w + 2]);
    }
    if (nnz > INT_MAX) return fail(result, SpMVError::INVALID_DIMENSION);
    (void)hipEventElapsedTime(&result->symbolic_ms, ev.e[0], ev.e[1]);

    // ---- numeric pass ----
    DeviceCsrArrays c;
    if (c.alloc_entries(nnz) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    if (nnz > 0) {
        args.c_rp = counts.get();
        args.c_ci = c.col_indices;
        args.c_va = c.values;
        ok = hipEventRecord(ev.e[2], s) == hipSuccess && launch_add<WRITE>(lanes, grid, args, s) == hipSuccess &&
             hipEventRecord(ev.e[3], s) == hipSuccess;
        ok = hipStreamSynchronize(s) == hipSuccess && ok;
        if (!ok) {
            c.release();
            return fail(result, SpMVError::KERNEL_LAUNCH);
        }
        (void)hipEventElapsedTime(&result->numeric_ms, ev.e[2], ev.e[3]);
        ++result->launches;
    }
    c.row_ptrs = counts.release();
    csr_adopt_device(C, m, n, static_cast<int>(nnz), &c);
    result->nnz = static_cast<int>(nnz);
    result->common = static_cast<int>(common);
    result->max_row_nnz = static_cast<int>(longest);
    return 0;
}

int add_refill(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B, CsrAddResult* result,
               hipStream_t s) {
    *result = CsrAddResult();
    const int status = add_check(C, A, B, true);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    const TraceRange range("spmv:csr_add_numeric");
    const int m = A->num_rows;
    const int lanes = add_lanes_for(A, B);
    result->lanes = lanes;
    result->nnz = C->nnz;
    if (m == 0) return 0;                 // (no rows: nnz == 0 everywhere, by check 4)

    DevBuf<int> flag;
    if (dev_alloc(&flag, 1) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    AddArgs args{};
    args.A = view_of(A);
    args.B = view_of(B);
    args.m = m;
    args.n = A->num_cols;
    args.alpha = alpha;
    args.beta = beta;
    args.c_rp = C->d_row_ptrs;
    args.c_ci = C->d_col_indices;
    args.c_va = C->d_values;
    args.c_nnz = C->nnz;
    args.flag = flag.get();
    EventPair& ev = thread_events();
    int bad = 0;
    bool ok = ev.start && ev.stop && hipMemsetAsync(flag.get(), 0, sizeof(int), s) == hipSuccess &&
              hipEventRecord(ev.start, s) == hipSuccess &&
              launch_add<REFILL>(lanes, capped_grid(m, kBlock / lanes), args, s) == hipSuccess &&
              hipEventRecord(ev.stop, s) == hipSuccess &&
              hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    if (!ok) return fail(result, SpMVError::KERNEL_LAUNCH);
    result->launches = 1;
    if (bad) return fail(result, SpMVError::INVALID_FORMAT);
    (void)hipEventElapsedTime(&result->numeric_ms, ev.start, ev.stop);
    csr_invalidate_gpu_cache(C);          // a tiled plan, transpose or schedule built from the old values
    return 0;
}

} // namespace

} // namespace csr_ops
} // namespace detail

int csr_add(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B, CsrAddResult* result) {
    CsrAddResult local;
    return detail::csr_ops::add_build(C, alpha, A, beta, B, result ? result : &local, detail::current_stream());
}

int csr_add_numeric(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B,
                    CsrAddResult* result) {
    CsrAddResult local;
    return detail::csr_ops::add_refill(C, alpha, A, beta, B, result ? result : &local, detail::current_stream());
}

int csr_scale_gpu(CSRMatrix* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out) {
    using namespace detail;
    float* out = nullptr;
    bool in_place = false;
    const int status = csr_ops::scale_check(A, d_row_scale, d_col_scale, d_values_out, &out, &in_place);
    if (status != 0) return status;
    if (A->num_rows == 0) return 0;
    hipStream_t s = current_stream();
    const int checked = structure_checked(A, s);
    if (checked != 0) return checked;
    if (A->nnz == 0) return 0;
    if (in_place) csr_invalidate_gpu_cache(A);      // a tiled plan, transpose or schedule built from the old values
    csr_ops::csr_scale_kernel<<<dev::vec_grid(A->nnz), dev::kBlock, 0, s>>>(
        A->d_row_ptrs, A->d_col_indices, A->d_values, A->num_rows, A->nnz, d_row_scale, d_col_scale, out);
    return stream_finished(s);
}

int csr_diagonal_gpu(const CSRMatrix* A, float* d_diag) {
    using namespace detail;
    const int status = csr_ops::diagonal_check(A, d_diag);
    if (status != 0) return status;
    if (A->num_rows == 0) return 0;
    hipStream_t s = current_stream();
    const int checked = structure_checked(A, s);
    if (checked != 0) return checked;
    csr_ops::csr_diagonal_kernel<<<dev::vec_grid(A->num_rows), dev::kBlock, 0, s>>>(
        A->num_rows, A->d_row_ptrs, A->d_col_indices, A->d_values, d_diag);
    return stream_finished(s);
}

int csr_diag_matrix_gpu(CSRMatrix* D, int n, const float* d_diag) {
    using namespace detail;
    const int status = csr_ops::diag_matrix_check(D, n);
    if (status != 0) return status;
    DeviceCsrArrays d;
    const ReleaseOnExit release_d{&d};
    if (d.alloc(static_cast<long long>(n) + 1, n) != hipSuccess) return code(SpMVError::CUDA_MALLOC);
    hipStream_t s = current_stream();
    csr_ops::csr_diag_matrix_kernel<<<dev::vec_grid(static_cast<long long>(n) + 1), dev::kBlock, 0, s>>>(
        n, d_diag, d.row_ptrs, d.col_indices, d.values);
    const int done = stream_finished(s);
    if (done != 0) return done;
    csr_adopt_device(D, n, n, n, &d);
    return 0;
}

} // namespace spmv
