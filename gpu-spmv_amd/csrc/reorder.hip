// reorder.hip — multicolour reordering on the device (include/spmv/reorder.h).
//
//   csr_color        Jones-Plassmann in rounds.  A round is one launch: 1-64 lanes share a row, walk its entries (and
//                    those of the same row of A^T), recompute each neighbour's priority from its index and load its
//                    colour once: negative = a higher-priority neighbour is still uncoloured and the vertex waits;
//                    otherwise the colour goes into a 64-bit window of forbidden colours that is OR-folded across the
//                    row's lanes.  The colours are updated in place: a vertex takes its colour only when every
//                    higher-priority neighbour has been seen coloured, and a colour, once written, never changes, so
//                    which writes of the current round a vertex happens to see changes the round it colours in and
//                    never the colour.  The only atomic is one add per workgroup to the count of vertices left.
//   color_ordering   the stable counting sort by colour IS the transpose of the n x num_colors matrix with one entry
//                    per row: transpose_build's row pointers are the colour pointers, its column indices the ordering.
//   csr_permute_gpu  row lengths gathered through the row permutation, scanned, then every row fetches its entries
//                    through the column relabelling and stores each at its rank by comparison on (new column,
//                    position): a slice of 8 lanes, a wavefront, or a workgroup with the new columns in LDS, by row
//                    length; a matrix with a row past the LDS class is relabelled and transposed twice.
//   permute_gather   one element per thread.
// No kernel here waits for another workgroup; none uses an atomic on a value.
#include "reorder_impl.h"
#include "solver_common.h"

#include <climits>
#include <vector>

namespace spmv {
namespace detail {
namespace reorder {

namespace {

using dev::block_max;
using dev::capped_grid;
using dev::group_or;
using dev::kBlock;
using dev::vec_grid;
using dev::with_lanes;

constexpr int kInfoGrid = 1024;         // workgroups (and partial slots) of the reductions read back by the host

// the device state of one colouring; remaining[r % 3] = vertices still uncoloured after round r
struct ColorState {
    int remaining[3];
    int rounds;          // rounds that found something to do
    int num_colors;
};

// ---- colouring ----
__global__ __launch_bounds__(kBlock) void color_init_kernel(int n, int* __restrict__ colors,
                                                            ColorState* __restrict__ state) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        colors[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->remaining[0] = 0;
        state->remaining[1] = 0;
        state->remaining[2] = n;       // "after round -1"
        state->rounds = 0;
        state->num_colors = 0;
    }
}

// One round.  `colors` is read and written in place (see the head of this file); trp / tci: the pattern of A^T, or
// null when the caller promised a symmetric pattern.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void color_round_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, const int* __restrict__ trp,
                        const int* __restrict__ tci, unsigned seed, int* colors, ColorState* state, int round) {
    if (state->remaining[(round + 2) % 3] == 0) {                 // nothing was left after the round before:
        if (blockIdx.x == 0 && threadIdx.x == 0) state->remaining[round % 3] = 0;     // nor is after this one
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state->remaining[(round + 1) % 3] = 0;                    // the next round's count (last read a round ago)
        state->rounds = round + 1;
    }
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    int left = 0;
    for (long long row = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; row < n;
         row += static_cast<long long>(gridDim.x) * kRows) {
        const int v = static_cast<int>(row);
        if (colors[v] >= 0) continue;
        for (int base = 0;; base += 64) {
            unsigned lo = 0u, hi = 0u, blocked = 0u;
            auto walk = [&](const int* __restrict__ ptr, const int* __restrict__ col) {
                const int end = ptr[v + 1];
                for (int j = ptr[v] + lane; j < end; j += LANES) {
                    const int u = col[j];
                    if (u == v || !higher_priority(u, v, seed)) continue;
                    const int c = colors[u];                      // the one gather of the round
                    if (c < 0) {
                        blocked = 1u;
                    } else {
                        const unsigned d = static_cast<unsigned>(c - base);      // c < base wraps past 63
                        if (d < 32u) lo |= 1u << d;
                        else if (d < 64u) hi |= 1u << (d - 32u);
                    }
                }
            };
            walk(rp, ci);
            if (trp) walk(trp, tci);
            lo = group_or<LANES>(lo);
            hi = group_or<LANES>(hi);
            blocked = group_or<LANES>(blocked);
            if (blocked) {
                left += lane == 0;
                break;
            }
            const unsigned long long open = ~((static_cast<unsigned long long>(hi) << 32) | lo);
            if (open != 0ull) {
                if (lane == 0) colors[v] = base + __builtin_ctzll(open);
                break;
            }
            // the window [base, base + 64) is full: the next one, over the same row
        }
    }
    __shared__ int s_left[kBlock / 64];
    for (int off = 32; off > 0; off >>= 1) left += __shfl_xor(left, off, 64);
    if ((threadIdx.x & 63) == 0) s_left[threadIdx.x >> 6] = left;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBlock / 64; ++w) total += s_left[w];
        if (total > 0) atomicAdd(&state->remaining[round % 3], total);
    }
}

// partial[b] = the largest value workgroup b saw (values >= -1)
__global__ __launch_bounds__(kBlock) void max_partial_kernel(long long n, const int* __restrict__ data,
                                                             int* __restrict__ partial) {
    int m = -1;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        m = max(m, data[i]);
    }
    m = block_max(m);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(kBlock) void color_count_kernel(const int* __restrict__ partial, int count,
                                                             ColorState* __restrict__ state) {
    int m = -1;
    for (int i = threadIdx.x; i < count; i += kBlock) m = max(m, partial[i]);
    m = block_max(m);
    if (threadIdx.x == 0) state->num_colors = m + 1;
}

// ---- ordering ----
__global__ __launch_bounds__(kBlock) void ordering_kernel(int n, const int* __restrict__ sorted, int* __restrict__ perm,
                                                          int* __restrict__ inverse) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int old = sorted[i];
        perm[i] = old;
        inverse[old] = static_cast<int>(i);
    }
}

// ---- permutation ----
// info[0]: A's structure is bad (enqueue_validate of csr_build.hip); info[1]: an array is not a permutation;
// info[2 + b]: the longest row workgroup b of permute_lengths_kernel saw
__global__ __launch_bounds__(kBlock) void permute_mark_kernel(const int* __restrict__ row_perm, int rows,
                                                              const int* __restrict__ col_inverse, int cols,
                                                              int* __restrict__ seen_rows, int* __restrict__ seen_cols,
                                                              int* __restrict__ info) {
    const long long work = max(rows, cols);
    bool bad = false;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < work;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        if (row_perm && i < rows) {
            const int p = row_perm[i];
            if (p < 0 || p >= rows) bad = true; else seen_rows[p] = 1;
        }
        if (col_inverse && i < cols) {
            const int q = col_inverse[i];
            if (q < 0 || q >= cols) bad = true; else seen_cols[q] = 1;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) info[1] = 1;
}

// new_rp[i] = the length of B's row i (new_rp[rows] = 0: the scan turns it into nnz); an index no entry of its array
// named means that another was repeated
__global__ __launch_bounds__(kBlock) void permute_lengths_kernel(const int* __restrict__ rp,
                                                                 const int* __restrict__ row_perm, int rows, int cols,
                                                                 const int* __restrict__ seen_rows,
                                                                 const int* __restrict__ seen_cols,
                                                                 int* __restrict__ new_rp, int* __restrict__ info) {
    const long long work = max(static_cast<long long>(rows) + 1, static_cast<long long>(cols));
    bool bad = false;
    int longest = 0;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < work;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        if (i < rows) {
            if (seen_rows && !seen_rows[i]) bad = true;
            const int p = row_perm ? row_perm[i] : static_cast<int>(i);
            const int len = p >= 0 && p < rows ? rp[p + 1] - rp[p] : 0;
            new_rp[i] = len;
            longest = max(longest, len);
        } else if (i == rows) {
            new_rp[i] = 0;
        }
        if (seen_cols && i < cols && !seen_cols[i]) bad = true;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) info[1] = 1;
    longest = block_max(longest);
    if (threadIdx.x == 0) info[2 + blockIdx.x] = longest;
}

// Rows of B with more than `above` and at most LANES entries, one per aligned slice of LANES lanes: every lane holds
// one entry and counts the entries that come before it in (new column, position) order.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void permute_rows_kernel(int rows, int above, const int* __restrict__ rp, const int* __restrict__ ci,
                         const unsigned* __restrict__ va, const int* __restrict__ row_perm,
                         const int* __restrict__ col_inverse, const int* __restrict__ new_rp, int* __restrict__ new_ci,
                         unsigned* __restrict__ new_va) {
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    for (long long i = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; i < rows;
         i += static_cast<long long>(gridDim.x) * kRows) {
        const int begin = new_rp[i];
        const int len = new_rp[i + 1] - begin;
        if (len <= above || len > LANES) continue;
        const int src = rp[row_perm ? row_perm[i] : static_cast<int>(i)];
        const bool mine = lane < len;
        int c = INT_MAX;
        unsigned val = 0u;
        if (mine) {
            const int old = ci[src + lane];
            c = col_inverse ? col_inverse[old] : old;
            val = va[src + lane];
        }
        int rank = 0;
        for (int j = 0; j < len; ++j) {
            const int cj = __shfl(c, j, LANES);
            rank += (cj < c || (cj == c && j < lane)) ? 1 : 0;
        }
        if (mine) {
            new_ci[begin + rank] = c;
            new_va[begin + rank] = val;
        }
    }
}

// Rows of B with more than kPermuteWave and at most kPermuteLds entries, one workgroup per row with the row's new
// columns in LDS.  A workgroup takes 256 consecutive rows at a time and walks those of them that are in the class.
__global__ __launch_bounds__(kBlock)
void permute_long_rows_kernel(int rows, const int* __restrict__ rp, const int* __restrict__ ci,
                              const unsigned* __restrict__ va, const int* __restrict__ row_perm,
                              const int* __restrict__ col_inverse, const int* __restrict__ new_rp,
                              int* __restrict__ new_ci, unsigned* __restrict__ new_va) {
    __shared__ int s_col[kPermuteLds];
    __shared__ int s_long[kBlock];
    for (long long first = static_cast<long long>(blockIdx.x) * kBlock; first < rows;
         first += static_cast<long long>(gridDim.x) * kBlock) {
        const long long mine = first + threadIdx.x;
        const int my_len = mine < rows ? new_rp[mine + 1] - new_rp[mine] : 0;
        s_long[threadIdx.x] = my_len > kPermuteWave && my_len <= kPermuteLds;
        __syncthreads();
        for (int r = 0; r < kBlock; ++r) {
            if (!s_long[r]) continue;                             // the same for every thread
            const long long i = first + r;
            const int begin = new_rp[i];
            const int len = new_rp[i + 1] - begin;
            const int src = rp[row_perm ? row_perm[i] : static_cast<int>(i)];
            for (int e = threadIdx.x; e < len; e += kBlock) {
                const int old = ci[src + e];
                s_col[e] = col_inverse ? col_inverse[old] : old;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < len; e += kBlock) {
                const int c = s_col[e];
                int rank = 0;
                for (int j = 0; j < len; ++j) {
                    const int cj = s_col[j];                      // one address per step: a broadcast
                    rank += (cj < c || (cj == c && j < e)) ? 1 : 0;
                }
                new_ci[begin + rank] = c;
                new_va[begin + rank] = va[src + e];
            }
            __syncthreads();
        }
        __syncthreads();
    }
}

// The rows relabelled and left in A's storage order, one wavefront per row: the input of the two transposes
__global__ __launch_bounds__(kBlock)
void permute_relabel_kernel(int rows, const int* __restrict__ rp, const int* __restrict__ ci,
                            const unsigned* __restrict__ va, const int* __restrict__ row_perm,
                            const int* __restrict__ col_inverse, const int* __restrict__ new_rp,
                            int* __restrict__ new_ci, unsigned* __restrict__ new_va) {
    const int lane = threadIdx.x & 63;
    for (long long i = static_cast<long long>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6); i < rows;
         i += static_cast<long long>(gridDim.x) * (kBlock / 64)) {
        const int begin = new_rp[i];
        const int len = new_rp[i + 1] - begin;
        const int src = rp[row_perm ? row_perm[i] : static_cast<int>(i)];
        for (int e = lane; e < len; e += 64) {
            const int old = ci[src + e];
            new_ci[begin + e] = col_inverse ? col_inverse[old] : old;
            new_va[begin + e] = va[src + e];
        }
    }
}

// ---- gather ----
__global__ __launch_bounds__(kBlock) void gather_kernel(float* __restrict__ out, int ldo, const float* __restrict__ in,
                                                        int ldi, const int* __restrict__ index, long long n, int k) {
    const long long total = n * k;
    for (long long e = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; e < total;
         e += static_cast<long long>(gridDim.x) * kBlock) {
        const long long i = e / k;
        const int j = static_cast<int>(e - i * k);
        out[i * ldo + j] = in[static_cast<long long>(index[i]) * ldi + j];
    }
}

// the colouring on `s`; the checks of color_check have passed and A has rows
int color(const CSRMatrix* A, int* d_colors, const ColorConfig& cfg, ColorResult* result, hipStream_t s) {
    const int n = A->num_rows;
    solver::Workspace<ColorState> ws;
    DevBuf<int> partial;
    if (!ws.allocate(0, 0) || dev_alloc(&partial, dev::kVecBlocks) != hipSuccess) {
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    // the device pass over the structure, before anything walks it and before d_colors is written
    const int checked = structure_checked(A, s);
    if (checked == 0 || checked == code(SpMVError::INVALID_FORMAT)) result->launches = 1;    // the check ran
    if (checked != 0) return fail(result, static_cast<SpMVError>(checked));

    DeviceCsrArrays at;
    const ReleaseOnExit release_at{&at};
    if (!cfg.symmetric_pattern) {
        const int status = transpose_build(A, &at, s);
        if (status != 0) {
            result->error_code = status;
            return status;
        }
    }

    const TraceRange range("spmv:csr_color");
    const int lanes = cfg.lanes_per_row != 0
                          ? cfg.lanes_per_row
                          : pick_lanes_per_row(static_cast<float>(A->nnz) / static_cast<float>(n));
    const int grid = capped_grid(n, kBlock / lanes);
    EventPair& ev = thread_events();
    if (!ev.start || !ev.stop || hipEventRecord(ev.start, s) != hipSuccess) return fail(result, SpMVError::KERNEL_LAUNCH);
    color_init_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, d_colors, ws.state);
    bool ok = hipGetLastError() == hipSuccess;
    ++result->launches;
    ok = ok && solver::run_rounds(n, ws, s, [&](int round) {
        ++result->launches;
        return with_lanes(lanes, [&](auto L) {
            color_round_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(
                n, A->d_row_ptrs, A->d_col_indices, at.row_ptrs, at.col_indices, cfg.seed, d_colors, ws.state, round);
            return hipGetLastError();
        });
    });
    if (ok) {
        const int blocks = vec_grid(n);
        max_partial_kernel<<<blocks, kBlock, 0, s>>>(n, d_colors, partial.get());
        color_count_kernel<<<1, kBlock, 0, s>>>(partial.get(), blocks, ws.state);
        ok = hipGetLastError() == hipSuccess;
        result->launches += 2;
    }
    if (!ws.finish_timed(ok, ev, s, &result->elapsed_ms)) {
        (void)hipStreamSynchronize(s);                            // the transpose is freed after the last round
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    result->rounds = ws.pinned[0].rounds;
    result->num_colors = ws.pinned[0].num_colors;
    return 0;
}

int ordering(int n, const int* d_colors, int num_colors, int* d_perm, int* d_inverse, int* color_ptr, hipStream_t s) {
    DevBuf<int> iota;
    const long long count = static_cast<long long>(n) + 1;
    if (dev_alloc(&iota, count) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    if (launch_iota(count, iota.get(), vec_grid(count), s) != hipSuccess) return code(SpMVError::KERNEL_LAUNCH);
    // the n x num_colors matrix with the entry (i, colour[i]) in row i: row c of its transpose lists the vertices of
    // colour c in ascending order.  The values are never looked at: the colours stand in for them.
    CSRMatrix byrow{};
    byrow.num_rows = n;
    byrow.num_cols = num_colors;
    byrow.nnz = n;
    byrow.d_row_ptrs = iota.get();
    byrow.d_col_indices = const_cast<int*>(d_colors);
    byrow.d_values = reinterpret_cast<float*>(const_cast<int*>(d_colors));
    DeviceCsrArrays bycolor;
    const int status = transpose_build(&byrow, &bycolor, s);
    if (status == code(SpMVError::INVALID_FORMAT)) return code(SpMVError::INVALID_ARGUMENT);    // a colour out of range
    if (status != 0) return status;
    ordering_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, bycolor.col_indices, d_perm, d_inverse);
    bool ok = hipGetLastError() == hipSuccess;
    if (ok && color_ptr) {
        ok = hipMemcpyAsync(color_ptr, bycolor.row_ptrs, (static_cast<size_t>(num_colors) + 1) * sizeof(int),
                            hipMemcpyDeviceToHost, s) == hipSuccess;
    }
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    bycolor.release();
    if (!ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}

int permute(CSRMatrix* B, const CSRMatrix* A, const int* d_row_perm, const int* d_col_inverse, hipStream_t s) {
    const int rows = A->num_rows, cols = A->num_cols, nnz = A->nnz;
    const TraceRange range("spmv:csr_permute_gpu");
    DeviceCsrArrays out;
    const ReleaseOnExit release_out{&out};
    const size_t ptr_bytes = (static_cast<size_t>(rows) + 1) * sizeof(int);
    if (out.alloc(static_cast<long long>(rows) + 1, 0) != hipSuccess) return code(SpMVError::CUDA_MALLOC);
    if (rows == 0) {                                              // (nnz == 0: permute_check)
        if (hipMemsetAsync(out.row_ptrs, 0, ptr_bytes, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            return code(SpMVError::KERNEL_LAUNCH);
        }
        csr_adopt_device(B, rows, cols, 0, &out);
        return 0;
    }

    // ---- the device checks and the row lengths, one read-back ----
    const int grid = capped_grid(std::max<long long>(static_cast<long long>(rows) + 1, cols), kBlock, kInfoGrid);
    std::vector<int> info(2 + static_cast<size_t>(grid));
    DevBuf<int> d_info, seen_rows, seen_cols;
    bool got = dev_alloc(&d_info, static_cast<long long>(info.size())) == hipSuccess &&
               (!d_row_perm || dev_alloc(&seen_rows, rows) == hipSuccess) &&
               (!d_col_inverse || dev_alloc(&seen_cols, cols) == hipSuccess);
    if (!got) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    bool ok = hipMemsetAsync(d_info.get(), 0, info.size() * sizeof(int), s) == hipSuccess &&
              (!seen_rows || hipMemsetAsync(seen_rows.get(), 0, static_cast<size_t>(rows) * sizeof(int), s) == hipSuccess) &&
              (!seen_cols || cols == 0 ||
               hipMemsetAsync(seen_cols.get(), 0, static_cast<size_t>(cols) * sizeof(int), s) == hipSuccess);
    if (ok) {
        ok = enqueue_validate(A, d_info.get(), s) == hipSuccess;
        if (d_row_perm || d_col_inverse) {
            permute_mark_kernel<<<capped_grid(std::max(rows, cols), kBlock), kBlock, 0, s>>>(
                d_row_perm, rows, d_col_inverse, cols, seen_rows.get(), seen_cols.get(), d_info.get());
        }
        permute_lengths_kernel<<<grid, kBlock, 0, s>>>(A->d_row_ptrs, d_row_perm, rows, cols, seen_rows.get(),
                                                       seen_cols.get(), out.row_ptrs, d_info.get());
        ok = ok && hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(info.data(), d_info.get(), info.size() * sizeof(int), hipMemcpyDeviceToHost, s) ==
                 hipSuccess;
    }
    if (hipStreamSynchronize(s) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    if (info[0]) return code(SpMVError::INVALID_FORMAT);
    if (info[1]) return code(SpMVError::INVALID_ARGUMENT);
    int longest = 0;
    for (int b = 0; b < grid; ++b) longest = std::max(longest, info[2 + b]);

    // ---- row pointers: the scan of the lengths ----
    const std::vector<long long> levels = device_scan_levels(static_cast<long long>(rows) + 1);
    DevBuf<int> sums;
    if (dev_alloc(&sums, device_scan_sums(levels)) != hipSuccess || out.alloc_entries(nnz) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    ok = device_exclusive_scan(out.row_ptrs, levels, sums.get(), s) == hipSuccess;

    // ---- the entries, by row length ----
    const unsigned* va = reinterpret_cast<const unsigned*>(A->d_values);
    unsigned* new_va = reinterpret_cast<unsigned*>(out.values);
    if (ok && nnz > 0 && longest <= kPermuteLds) {
        permute_rows_kernel<kPermuteSlice><<<capped_grid(rows, kBlock / kPermuteSlice), kBlock, 0, s>>>(
            rows, 0, A->d_row_ptrs, A->d_col_indices, va, d_row_perm, d_col_inverse, out.row_ptrs, out.col_indices,
            new_va);
        if (longest > kPermuteSlice) {
            permute_rows_kernel<kPermuteWave><<<capped_grid(rows, kBlock / kPermuteWave), kBlock, 0, s>>>(
                rows, kPermuteSlice, A->d_row_ptrs, A->d_col_indices, va, d_row_perm, d_col_inverse, out.row_ptrs,
                out.col_indices, new_va);
        }
        if (longest > kPermuteWave) {
            permute_long_rows_kernel<<<capped_grid(rows, kBlock), kBlock, 0, s>>>(
                rows, A->d_row_ptrs, A->d_col_indices, va, d_row_perm, d_col_inverse, out.row_ptrs, out.col_indices,
                new_va);
        }
        ok = hipGetLastError() == hipSuccess;
    } else if (ok && nnz > 0) {
        // A row past the LDS class: the whole matrix relabelled in A's storage order, then transposed twice.  The
        // stable sort of the first transpose orders every column by row, that of the second every row by (column,
        // position): the order the ranking kernels produce.
        permute_relabel_kernel<<<capped_grid(rows, kBlock / 64), kBlock, 0, s>>>(
            rows, A->d_row_ptrs, A->d_col_indices, va, d_row_perm, d_col_inverse, out.row_ptrs, out.col_indices, new_va);
        if (hipGetLastError() != hipSuccess) return code(SpMVError::KERNEL_LAUNCH);
        CSRMatrix relabelled{};
        relabelled.num_rows = rows;
        relabelled.num_cols = cols;
        relabelled.nnz = nnz;
        relabelled.d_row_ptrs = out.row_ptrs;
        relabelled.d_col_indices = out.col_indices;
        relabelled.d_values = out.values;
        DeviceCsrArrays first;
        int status = transpose_build(&relabelled, &first, s);
        if (status != 0) return status;
        CSRMatrix turned{};
        turned.num_rows = cols;
        turned.num_cols = rows;
        turned.nnz = nnz;
        turned.d_row_ptrs = first.row_ptrs;
        turned.d_col_indices = first.col_indices;
        turned.d_values = first.values;
        DeviceCsrArrays second;
        status = transpose_build(&turned, &second, s);
        first.release();
        if (status != 0) return status;
        out.release();
        out = second;
    }
    if (hipStreamSynchronize(s) != hipSuccess || !ok) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    csr_adopt_device(B, rows, cols, nnz, &out);          // B owns them now
    return 0;
}

} // namespace

} // namespace reorder

} // namespace detail

ColorResult csr_color(const CSRMatrix* A, int* d_colors, const ColorConfig* config) {
    using namespace detail;
    ColorResult result;
    const ColorConfig defaults;
    const ColorConfig& cfg = config ? *config : defaults;
    bool nothing = false;
    result.error_code = reorder::color_check(A, d_colors, cfg, &nothing);
    if (result.error_code != 0 || nothing) return result;
    reorder::color(A, d_colors, cfg, &result, current_stream());
    return result;
}

int color_ordering(int n, const int* d_colors, int num_colors, int* d_perm, int* d_inverse, int* color_ptr) {
    using namespace detail;
    bool nothing = false;
    const int status = reorder::ordering_check(n, d_colors, num_colors, d_perm, d_inverse, &nothing);
    if (status != 0) return status;
    if (nothing) {
        if (color_ptr) std::fill(color_ptr, color_ptr + num_colors + 1, 0);
        return 0;
    }
    return reorder::ordering(n, d_colors, num_colors, d_perm, d_inverse, color_ptr, current_stream());
}

int csr_permute_gpu(CSRMatrix* B, const CSRMatrix* A, const int* d_row_perm, const int* d_col_inverse) {
    using namespace detail;
    const int status = reorder::permute_check(B, A);
    if (status != 0) return status;
    return reorder::permute(B, A, d_row_perm, d_col_inverse, current_stream());
}

int permute_gather_async(float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k,
                         hipStream_t stream) {
    using namespace detail;
    bool nothing = false;
    const int status = reorder::gather_check(d_out, ldo, d_in, ldi, d_index, n, k, &nothing);
    if (status != 0 || nothing) return status;
    reorder::gather_kernel<<<dev::capped_grid(static_cast<long long>(n) * k, reorder::kBlock), reorder::kBlock, 0,
                             stream>>>(d_out, ldo, d_in, ldi, d_index, n, k);
    return hipGetLastError() == hipSuccess ? 0 : code(SpMVError::KERNEL_LAUNCH);
}

int permute_gather(float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k) {
    using namespace detail;
    hipStream_t s = current_stream();
    const int status = permute_gather_async(d_out, ldo, d_in, ldi, d_index, n, k, s);
    if (status != 0 || n == 0) return status;
    return stream_finished(s);
}

ColorResult multicolor_reorder(CSRMatrix* B, const CSRMatrix* A, int* d_perm, int* d_inverse,
                               const ColorConfig* config) {
    using namespace detail;
    ColorResult result;
    if (!B || !A || !d_perm || !d_inverse || B == A) {
        result.error_code = code(SpMVError::INVALID_ARGUMENT);
        return result;
    }
    const ColorConfig defaults;
    const ColorConfig& cfg = config ? *config : defaults;
    DevBuf<int> colors;
    if (dev_alloc(&colors, A->num_rows > 0 ? A->num_rows : 1) != hipSuccess) {
        (void)hipGetLastError();
        result.error_code = code(SpMVError::CUDA_MALLOC);
        return result;
    }
    bool nothing = false;
    result.error_code = reorder::color_check(A, colors.get(), cfg, &nothing);
    if (result.error_code != 0) return result;
    hipStream_t s = current_stream();
    if (!nothing && reorder::color(A, colors.get(), cfg, &result, s) != 0) return result;
    result.error_code = color_ordering(A->num_rows, colors.get(), result.num_colors, d_perm, d_inverse, nullptr);
    if (result.error_code != 0) return result;
    result.error_code = csr_permute_gpu(B, A, d_perm, d_inverse);
    return result;
}

} // namespace spmv
