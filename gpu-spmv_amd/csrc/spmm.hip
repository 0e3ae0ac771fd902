// spmm.hip — multi-vector SpMV (Y = A * X for k right-hand sides, csrmm / SpMM) for gfx950.
//
// X (num_cols x k) and Y (num_rows x k) are row-major with leading dimensions ldx / ldy >= k.
// Every kernel reads each (column, value) pair of the matrix once per column chunk and turns the
// k 4-byte gathers of a single-vector call into one contiguous read of a row slice of X
// (16-byte loads when ldx % 4 == 0 and X is 16-byte aligned).  All offsets into X and Y are 64-bit.
//
//   csr_multi_rows_kernel<C>     a group of G lanes per row, each lane owning C consecutive columns;
//                                every lane walks the row's entries in storage order with separate
//                                multiply and add roundings: column j of Y is bit-identical to
//                                spmv_cpu_csr(A, X[:, j]).  SCALAR_CSR at every k, VECTOR_CSR at k > 4.
//   csr_multi_split_kernel<K, L> L lanes split a row's entries, K accumulators per lane, reduced by
//                                group_sum<L> (DPP).  VECTOR_CSR at k <= 4 and k == 8.
//   csr_multi_merge_*            merge-path: equal (rows + nnz) shares per workgroup, a CW-column chunk
//                                at a time, a k-wide segmented scan in LDS and k-wide carry slots added
//                                by a fix-up kernel in a fixed order.  MERGE_PATH.
// No floating-point atomics anywhere: results are bitwise reproducible from run to run.
#include "internal.h"
#include "device_common.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

namespace spmv {
namespace detail {

namespace {

using namespace dev;

// C consecutive floats of X's row `col`, starting at column j0; `w` of them exist (w < C: the remainder of k).
// `vec`: X's rows are 16-byte aligned at every multiple of 4 (ldx % 4 == 0, X aligned), so C % 4 == 0
// slices that are complete load as dwordx4.
template <int C>
__device__ __forceinline__ void load_slice(const float* __restrict__ X, long long ldx, int col, int j0, int w,
                                           bool vec, float (&out)[C]) {
    const float* p = X + static_cast<long long>(col) * ldx + j0;
    if constexpr (C % 4 == 0) {
        if (vec && w == C) {
#pragma unroll
            for (int q = 0; q < C; q += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(p + q);
                out[q] = v[0]; out[q + 1] = v[1]; out[q + 2] = v[2]; out[q + 3] = v[3];
            }
            return;
        }
    }
#pragma unroll
    for (int q = 0; q < C; ++q) out[q] = q < w ? p[q] : 0.0f;
}

template <int C>
__device__ __forceinline__ void store_slice(float* __restrict__ Y, long long ldy, long long row, int j0, int w,
                                            const float (&v)[C]) {
    float* p = Y + row * ldy + j0;
#pragma unroll
    for (int q = 0; q < C; ++q) {
        if (q < w) p[q] = v[q];
    }
}

// ---------------------------------------------------------------------------
// Column split (CPU summation order).  A workgroup of 256 lanes holds 256 / G row groups; lane `lane` of a
// group owns columns [jw + lane*C, jw + lane*C + C) of every column window jw (G*C columns per window).
// Entries are read four at a time through 16-byte loads (the same address for every lane of a group), the
// four slices of X are loaded before any of them is used, then added in storage order.
// ---------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kBlock)
void csr_multi_rows_kernel(int num_rows, long long nnz,
                           const int* __restrict__ row_ptrs,
                           const int* __restrict__ cols,
                           const float* __restrict__ vals,
                           const float* __restrict__ X, long long ldx,
                           float* __restrict__ Y, long long ldy,
                           int k, int group_log2, bool vec) {
    const int G = 1 << group_log2;
    const int lane = threadIdx.x & (G - 1);
    const int rows_per_block = kBlock >> group_log2;
    const long long slot = threadIdx.x >> group_log2;

    for (long long first = static_cast<long long>(blockIdx.x) * rows_per_block; first < num_rows;
         first += static_cast<long long>(gridDim.x) * rows_per_block) {
        const long long row = first + slot;
        if (row >= num_rows) break;
        const int begin = row_ptrs[row];
        const int end = row_ptrs[row + 1];
        for (int jw = 0; jw < k; jw += G * C) {
            const int j0 = jw + lane * C;
            const int w = min(C, k - j0);
            if (w <= 0) continue;
            float acc[C];
#pragma unroll
            for (int q = 0; q < C; ++q) acc[q] = 0.0f;
            for (long long p = begin & ~3; p < end; p += 4) {
                i32x4 c;
                f32x4 v;
                load4(cols, vals, p, nnz, c, v);
                bool mine[4];
                float xv[4][C];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    mine[e] = p + e >= begin && p + e < end;
                    // entries of neighbouring rows read X's row 0 and are never added (X may hold inf / nan)
                    load_slice<C>(X, ldx, mine[e] ? c[e] : 0, j0, w, vec, xv[e]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int q = 0; q < C; ++q) {
                        acc[q] = mine[e] ? __fadd_rn(acc[q], __fmul_rn(v[e], xv[e][q])) : acc[q];
                    }
                }
            }
            store_slice<C>(Y, ldy, row, j0, w, acc);
        }
    }
}

// ---------------------------------------------------------------------------
// Entry split (reorders a row's sum): L lanes per row, four entries per lane per step as row_partial_dot
// does, K accumulators per lane, each reduced with the DPP butterfly.
// ---------------------------------------------------------------------------
template <int K, int L>
__global__ __launch_bounds__(kBlock)
void csr_multi_split_kernel(int num_rows, long long nnz,
                            const int* __restrict__ row_ptrs,
                            const int* __restrict__ cols,
                            const float* __restrict__ vals,
                            const float* __restrict__ X, long long ldx,
                            float* __restrict__ Y, long long ldy, bool vec) {
    constexpr int kRowsPerBlock = kBlock / L;
    const int lane = threadIdx.x % L;
    const int slot = threadIdx.x / L;

    for (long long first = static_cast<long long>(blockIdx.x) * kRowsPerBlock; first < num_rows;
         first += static_cast<long long>(gridDim.x) * kRowsPerBlock) {
        const long long row = first + slot;
        float acc[K];
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = 0.0f;
        if (row < num_rows) {
            const int begin = row_ptrs[row];
            const int end = row_ptrs[row + 1];
            for (long long p = (begin & ~3) + lane * 4; p < end; p += L * 4) {
                i32x4 c;
                f32x4 v;
                load4(cols, vals, p, nnz, c, v);
                bool mine[4];
                float xv[4][K];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    mine[e] = p + e >= begin && p + e < end;
                    load_slice<K>(X, ldx, mine[e] ? c[e] : 0, 0, K, vec, xv[e]);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int q = 0; q < K; ++q) acc[q] = mine[e] ? __builtin_fmaf(v[e], xv[e][q], acc[q]) : acc[q];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] = group_sum<L>(acc[q]);
        if (lane == 0 && row < num_rows) store_slice<K>(Y, ldy, row, 0, K, acc);
    }
}

// ---------------------------------------------------------------------------
// MERGE_PATH, k columns.  The tile's row ends and (column, value) pairs are staged in LDS once; then, for
// every chunk of CW columns, each thread walks its kMultiItems merge items (gathering X's row slices),
// stores the rows it completes after its first, and the k-wide per-thread carries meet in a segmented
// inclusive scan (Hillis-Steele, fixed order).  The tile's own carry-out goes to k-wide slots that
// csr_multi_merge_fixup_kernel adds in tile order.
// ---------------------------------------------------------------------------
constexpr int kMultiItems = 7;                        // odd: conflict-free LDS walk
constexpr int kMultiTile = kBlock * kMultiItems;      // 1792 merge items per workgroup

__global__ __launch_bounds__(kBlock)
void csr_multi_merge_partition_kernel(int num_rows, int nnz, const int* __restrict__ row_ptrs,
                                      int num_tiles, int* __restrict__ tile_rows) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t > num_tiles) return;
    const long long total = static_cast<long long>(num_rows) + nnz;
    const long long diag = min(static_cast<long long>(t) * kMultiTile, total);
    // number of row-end items among the first `diag` merge items
    const int* row_end = row_ptrs + 1;
    long long lo = diag > nnz ? diag - nnz : 0;
    long long hi = diag < num_rows ? diag : num_rows;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (row_end[mid] <= diag - mid - 1) lo = mid + 1; else hi = mid;
    }
    tile_rows[t] = static_cast<int>(lo);
}

template <int CW>
__global__ __launch_bounds__(kBlock)
void csr_multi_merge_tile_kernel(int num_rows, int nnz,
                                 const int* __restrict__ row_ptrs,
                                 const int* __restrict__ cols,
                                 const float* __restrict__ vals,
                                 const float* __restrict__ X, long long ldx,
                                 float* __restrict__ Y, long long ldy, int k, bool vec,
                                 const int* __restrict__ tile_rows,
                                 int* __restrict__ carry_row,
                                 float* __restrict__ carry_val) {
    __shared__ int   s_row_end[kMultiTile + 1];
    __shared__ int   s_col[kMultiTile];
    __shared__ float s_v[kMultiTile];
    __shared__ int   s_key[kBlock];
    __shared__ float s_scan[2][CW][kBlock];

    const int tile = blockIdx.x;
    const int t = threadIdx.x;
    const long long total = static_cast<long long>(num_rows) + nnz;
    const long long diag0 = static_cast<long long>(tile) * kMultiTile;
    const long long diag1 = min(diag0 + kMultiTile, total);

    const int row0 = tile_rows[tile];
    const int row1 = tile_rows[tile + 1];
    const int nz0 = static_cast<int>(diag0 - row0);
    const int nz1 = static_cast<int>(diag1 - row1);
    const int n_rows = row1 - row0;
    const int n_nz = nz1 - nz0;

    for (int i = t; i <= n_rows; i += kBlock) {
        const int r = row0 + i;
        s_row_end[i] = r < num_rows ? row_ptrs[r + 1] : INT_MAX;
    }
    for (int i = t; i < n_nz; i += kBlock) {
        s_col[i] = cols[nz0 + i];
        s_v[i] = vals[nz0 + i];
    }
    __syncthreads();

    const int items = static_cast<int>(diag1 - diag0);
    const int d_begin = min(t * kMultiItems, items);
    const int d_end = min(d_begin + kMultiItems, items);
    int i0;
    {
        int lo = d_begin > n_nz ? d_begin - n_nz : 0;
        int hi = d_begin < n_rows ? d_begin : n_rows;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_row_end[mid] <= nz0 + (d_begin - mid - 1)) lo = mid + 1; else hi = mid;
        }
        i0 = lo;
    }
    const int j0 = d_begin - i0;

    for (int c0 = 0; c0 < k; c0 += CW) {
        const int w = min(CW, k - c0);
        int i = i0, j = j0;
        float running[CW], first_sum[CW];
#pragma unroll
        for (int q = 0; q < CW; ++q) running[q] = first_sum[q] = 0.0f;
        bool have_first = false;
        int first_row = 0;

        for (int step = d_begin; step < d_end; ++step) {
            if (nz0 + j < s_row_end[i]) {
                float xv[CW];
                load_slice<CW>(X, ldx, s_col[j], c0, w, vec, xv);
                const float v = s_v[j];
#pragma unroll
                for (int q = 0; q < CW; ++q) running[q] = __builtin_fmaf(v, xv[q], running[q]);
                ++j;
            } else {
                if (!have_first) {
                    have_first = true;
                    first_row = row0 + i;
#pragma unroll
                    for (int q = 0; q < CW; ++q) first_sum[q] = running[q];
                } else {
                    store_slice<CW>(Y, ldy, row0 + i, c0, w, running);
                }
#pragma unroll
                for (int q = 0; q < CW; ++q) running[q] = 0.0f;
                ++i;
            }
        }

        // segmented inclusive scan of the per-thread carries (key = the row left open)
        int cur = 0;
        s_key[t] = row0 + i;
#pragma unroll
        for (int q = 0; q < CW; ++q) s_scan[0][q][t] = running[q];
        __syncthreads();
#pragma unroll
        for (int off = 1; off < kBlock; off <<= 1) {
            const bool joins = t >= off && s_key[t - off] == s_key[t];
#pragma unroll
            for (int q = 0; q < CW; ++q) {
                const float v = s_scan[cur][q][t];
                s_scan[cur ^ 1][q][t] = joins ? s_scan[cur][q][t - off] + v : v;
            }
            cur ^= 1;
            __syncthreads();
        }

        if (have_first) {
            const bool carried = t > 0 && s_key[t - 1] == first_row;
            float out[CW];
#pragma unroll
            for (int q = 0; q < CW; ++q) out[q] = (carried ? s_scan[cur][q][t - 1] : 0.0f) + first_sum[q];
            store_slice<CW>(Y, ldy, first_row, c0, w, out);
        }
        if (t < w) carry_val[static_cast<long long>(tile) * k + c0 + t] = s_scan[cur][t][kBlock - 1];
        if (t == 0 && c0 == 0) carry_row[tile] = s_key[kBlock - 1];
        __syncthreads();     // s_key / s_scan are rewritten by the next chunk
    }
}

// one thread per (tile, column): the first tile of every run of equal carry rows sums the run left to
// right and adds it to Y once
__global__ __launch_bounds__(kBlock)
void csr_multi_merge_fixup_kernel(int num_rows, int num_tiles, int k,
                                  const int* __restrict__ carry_row,
                                  const float* __restrict__ carry_val,
                                  float* __restrict__ Y, long long ldy) {
    const long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
    if (idx >= static_cast<long long>(num_tiles) * k) return;
    const int tile = static_cast<int>(idx / k);
    const int col = static_cast<int>(idx % k);
    const int row = carry_row[tile];
    if (row >= num_rows) return;
    if (tile > 0 && carry_row[tile - 1] == row) return;
    float sum = carry_val[idx];
    for (int u = tile + 1; u < num_tiles && carry_row[u] == row; ++u) {
        sum += carry_val[static_cast<long long>(u) * k + col];
    }
    Y[static_cast<long long>(row) * ldy + col] += sum;
}

// nnz == 0: Y[i, 0:k] = 0, padding columns untouched
__global__ __launch_bounds__(kBlock)
void csr_multi_zero_kernel(int num_rows, int k, float* __restrict__ Y, long long ldy) {
    const long long n = static_cast<long long>(num_rows) * k;
    for (long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; idx < n;
         idx += static_cast<long long>(gridDim.x) * kBlock) {
        Y[(idx / k) * ldy + idx % k] = 0.0f;
    }
}

inline bool vec_ok(const float* X, int ldx) {
    return ldx % 4 == 0 && (reinterpret_cast<unsigned long long>(X) & 15) == 0;
}

template <int C>
hipError_t launch_rows(const CSRMatrix* A, const float* X, int ldx, float* Y, int ldy, int k, hipStream_t s) {
    const int lanes_needed = (k + C - 1) / C;
    int group_log2 = 0;
    while (group_log2 < 6 && (1 << group_log2) < lanes_needed) ++group_log2;
    const int grid = capped_grid(A->num_rows, kBlock >> group_log2);
    csr_multi_rows_kernel<C><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices,
                                                     A->d_values, X, ldx, Y, ldy, k, group_log2, vec_ok(X, ldx));
    return hipGetLastError();
}

template <int K, int L>
hipError_t launch_split(const CSRMatrix* A, const float* X, int ldx, float* Y, int ldy, hipStream_t s) {
    const int grid = capped_grid(A->num_rows, kBlock / L);
    csr_multi_split_kernel<K, L><<<grid, kBlock, 0, s>>>(A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices,
                                                         A->d_values, X, ldx, Y, ldy, vec_ok(X, ldx));
    return hipGetLastError();
}

template <int K>
hipError_t launch_split_lanes(const CSRMatrix* A, const float* X, int ldx, float* Y, int ldy, int lanes,
                              hipStream_t s) {
    return with_lanes(lanes, [&](auto L) { return launch_split<K, decltype(L)::value>(A, X, ldx, Y, ldy, s); });
}

int multi_num_tiles(const CSRMatrix* A) {
    const long long total = static_cast<long long>(A->num_rows) + A->nnz;
    return static_cast<int>((total + kMultiTile - 1) / kMultiTile);
}

void free_carry(CsrAux::MultiCarry& c) {
    if (c.row) (void)hipFree(c.row);
    if (c.val) (void)hipFree(c.val);
    c.row = nullptr;
    c.val = nullptr;
    c.cap_k = 0;
}

// (re)sizes one stream's carry pair for k columns; a pair that grows waits for its stream's earlier calls first
hipError_t fit_carry(CsrAux::MultiCarry& c, int num_tiles, int k, hipStream_t s) {
    if (c.row && c.cap_k >= k) return hipSuccess;
    if (c.row) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        free_carry(c);
    }
    hipError_t e = malloc_any_time(reinterpret_cast<void**>(&c.row), num_tiles * sizeof(int));
    if (e == hipSuccess) {
        e = malloc_any_time(reinterpret_cast<void**>(&c.val), static_cast<size_t>(num_tiles) * k * sizeof(float));
    }
    if (e != hipSuccess) {
        free_carry(c);
        return e;
    }
    c.cap_k = k;
    return hipSuccess;
}

hipError_t prepare_multi_merge_locked(const CSRMatrix* A, CsrAux* aux, hipStream_t s) {
    const int num_tiles = multi_num_tiles(A);
    if (num_tiles == 0) return hipSuccess;
    if (aux->multi_num_tiles == num_tiles && aux->d_multi_tile_rows) return hipSuccess;
    release_multi_merge(aux);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&aux->d_multi_tile_rows), (num_tiles + 1) * sizeof(int));
    if (e != hipSuccess) return e;
    csr_multi_merge_partition_kernel<<<(num_tiles + 1 + kBlock - 1) / kBlock, kBlock, 0, s>>>(
        A->num_rows, A->nnz, A->d_row_ptrs, num_tiles, aux->d_multi_tile_rows);
    e = hipGetLastError();
    // read by calls on any stream from now on: finished before it is announced (once per matrix)
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    aux->multi_num_tiles = num_tiles;
    return hipSuccess;
}

constexpr size_t kMaxMultiCarry = 8;      // streams that keep a k-wide carry pair with the matrix

// the carry pair of stream `s` (created or grown here), or nullptr past kMaxMultiCarry streams
CsrAux::MultiCarry* carry_for_stream(CsrAux* aux, int num_tiles, int k, hipStream_t s, hipError_t* err) {
    *err = hipSuccess;
    for (CsrAux::MultiCarry& c : aux->multi_carry) {
        if (c.stream == s) {
            *err = fit_carry(c, num_tiles, k, s);
            return *err == hipSuccess ? &c : nullptr;
        }
    }
    if (aux->multi_carry.size() >= kMaxMultiCarry) return nullptr;
    aux->multi_carry.push_back(CsrAux::MultiCarry{s, nullptr, nullptr, 0});
    *err = fit_carry(aux->multi_carry.back(), num_tiles, k, s);
    if (*err != hipSuccess) {
        aux->multi_carry.pop_back();
        return nullptr;
    }
    return &aux->multi_carry.back();
}

template <int CW>
hipError_t launch_merge_tiles(const CSRMatrix* A, const int* tile_rows, int num_tiles, const float* X, int ldx,
                              float* Y, int ldy, int k, int* carry_row, float* carry_val, hipStream_t s) {
    csr_multi_merge_tile_kernel<CW><<<num_tiles, kBlock, 0, s>>>(
        A->num_rows, A->nnz, A->d_row_ptrs, A->d_col_indices, A->d_values, X, ldx, Y, ldy, k, vec_ok(X, ldx),
        tile_rows, carry_row, carry_val);
    return hipGetLastError();
}

} // namespace

void release_multi_merge(CsrAux* aux) {
    if (aux->d_multi_tile_rows) (void)hipFree(aux->d_multi_tile_rows);
    aux->d_multi_tile_rows = nullptr;
    aux->multi_num_tiles = 0;
    for (CsrAux::MultiCarry& c : aux->multi_carry) free_carry(c);
    aux->multi_carry.clear();
}

hipError_t launch_csr_multi_zero(const CSRMatrix* A, float* d_Y, int ldy, int k, hipStream_t s) {
    csr_multi_zero_kernel<<<capped_grid(static_cast<long long>(A->num_rows) * k, kBlock), kBlock, 0, s>>>(
        A->num_rows, k, d_Y, ldy);
    return hipGetLastError();
}

hipError_t launch_csr_multi_rows(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                 hipStream_t s) {
    switch (k) {
        case 1:  return launch_rows<1>(A, d_X, ldx, d_Y, ldy, k, s);
        case 2:  return launch_rows<2>(A, d_X, ldx, d_Y, ldy, k, s);
        default: return launch_rows<4>(A, d_X, ldx, d_Y, ldy, k, s);
    }
}

hipError_t launch_csr_multi_vector(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                   hipStream_t s) {
    // k <= 4 and k == 8: lanes across a row's entries; otherwise lanes across columns (then in CPU order)
    if (k > 4 && k != 8) return launch_csr_multi_rows(A, d_X, ldx, d_Y, ldy, k, s);
    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / A->num_rows);
    switch (k) {
        case 1:  return launch_split_lanes<1>(A, d_X, ldx, d_Y, ldy, lanes, s);
        case 2:  return launch_split_lanes<2>(A, d_X, ldx, d_Y, ldy, lanes, s);
        case 3:  return launch_split_lanes<3>(A, d_X, ldx, d_Y, ldy, lanes, s);
        case 4:  return launch_split_lanes<4>(A, d_X, ldx, d_Y, ldy, lanes, s);
        default: return launch_split_lanes<8>(A, d_X, ldx, d_Y, ldy, lanes, s);
    }
}

hipError_t prepare_csr_multi_merge(const CSRMatrix* A, CsrAux* aux, int k, hipStream_t s) {
    if (!aux) return hipSuccess;
    std::lock_guard<std::mutex> guard(aux->multi_lock);
    hipError_t e = prepare_multi_merge_locked(A, aux, s);
    if (e != hipSuccess || aux->multi_num_tiles == 0) return e;
    (void)carry_for_stream(aux, aux->multi_num_tiles, k, s, &e);
    return e;
}

hipError_t launch_csr_multi_merge(const CSRMatrix* A, CsrAux* aux, const float* d_X, int ldx, float* d_Y,
                                  int ldy, int k, hipStream_t s) {
    const int num_tiles = multi_num_tiles(A);
    if (num_tiles == 0) return hipSuccess;
    // (the lock also keeps the tile + fix-up pair of one call together when two host threads share a stream)
    std::lock_guard<std::mutex> guard(aux->multi_lock);
    hipError_t e = prepare_multi_merge_locked(A, aux, s);
    if (e != hipSuccess) return e;

    int* carry_row = nullptr;
    float* carry_val = nullptr;
    CsrAux::MultiCarry* kept = carry_for_stream(aux, num_tiles, k, s, &e);
    if (e != hipSuccess) return e;
    bool borrowed = false;
    if (kept) {
        carry_row = kept->row;
        carry_val = kept->val;
    } else {
        // past kMaxMultiCarry streams: a pair from the stream-ordered allocator, given back behind this call
        if (hipMallocAsync(reinterpret_cast<void**>(&carry_row), num_tiles * sizeof(int), s) != hipSuccess ||
            hipMallocAsync(reinterpret_cast<void**>(&carry_val), static_cast<size_t>(num_tiles) * k * sizeof(float),
                           s) != hipSuccess) {
            (void)hipGetLastError();
            if (carry_row) (void)hipFreeAsync(carry_row, s);
            return hipErrorOutOfMemory;
        }
        borrowed = true;
    }

    // column chunks of 8 (2 x 8 accumulators per thread), narrower when k is
    const int* tile_rows = aux->d_multi_tile_rows;
    if (k >= 8) {
        e = launch_merge_tiles<8>(A, tile_rows, num_tiles, d_X, ldx, d_Y, ldy, k, carry_row, carry_val, s);
    } else if (k >= 4) {
        e = launch_merge_tiles<4>(A, tile_rows, num_tiles, d_X, ldx, d_Y, ldy, k, carry_row, carry_val, s);
    } else if (k >= 2) {
        e = launch_merge_tiles<2>(A, tile_rows, num_tiles, d_X, ldx, d_Y, ldy, k, carry_row, carry_val, s);
    } else {
        e = launch_merge_tiles<1>(A, tile_rows, num_tiles, d_X, ldx, d_Y, ldy, k, carry_row, carry_val, s);
    }
    if (e == hipSuccess) {
        const long long slots = static_cast<long long>(num_tiles) * k;
        csr_multi_merge_fixup_kernel<<<static_cast<int>((slots + kBlock - 1) / kBlock), kBlock, 0, s>>>(
            A->num_rows, num_tiles, k, carry_row, carry_val, d_Y, ldy);
        e = hipGetLastError();
    }
    if (borrowed) {
        (void)hipFreeAsync(carry_row, s);
        (void)hipFreeAsync(carry_val, s);
    }
    return e;
}

} // namespace detail
} // namespace spmv
