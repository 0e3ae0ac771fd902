// spgemm.hip — sparse matrix-matrix product C = A·B on the device (include/spmv/spgemm.h): validated,
// deterministic, bit-identical to spgemm_cpu_csr.  No float atomics, no global atomics, no waiting between workgroups.
//
// Two passes over the rows of C.  The symbolic pass counts every row's distinct columns; an exclusive scan of the
// counts gives C's row pointers; the numeric pass accumulates the values and writes each row in ascending column
// order.  In both a row goes to an accumulator class by its size (the symbolic pass knows min(products, n), the
// numeric pass the exact count): classes 1 .. 4 are open-addressing hash tables in LDS (int32 keys, -1 = empty, fp32
// values, slot = column mod slots, linear probing with wrap-around, at most half full), the last class a dense
// accumulator of n floats and an n-bit map in global scratch, one slice per workgroup.
//
// A lane group owns one row of C and walks A's entries one after another; its lanes take the entries of the current
// B row `lanes` at a time.  B's rows hold no repeated column, so no two lanes add into one accumulator within a step,
// and the steps follow each other in one wavefront's program order: every accumulator sees its additions in the
// order of the host loop.  Where a key lands in a table may differ from run to run (integer LDS atomicCAS claims the
// slots); the output is sorted by column, so that is invisible.
#include "internal.h"
#include "device_common.h"
#include "spmv/spgemm.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using dev::upper_bound;

constexpr int kThreads = 256;
constexpr int kMaxGrid = 4096;                // workgroups of any launch here; one flag each
constexpr int kSegments = kSpgemmClasses + 1; // class 0 (rows without products) .. the dense class
constexpr long long kDenseScratchCap = 256LL << 20;   // bytes of dense-class scratch by default
constexpr int kTableBudget = 64 * 1024;       // LDS bytes the tables of one workgroup may take (classes 1 .. 3)

static_assert(kSpgemmClasses == 5 && kSpgemmSlots[0] == 32 && kSpgemmSlots[1] == 256 && kSpgemmSlots[2] == 2048 &&
              kSpgemmSlots[3] == 16384, "slots_of() below restates the table");
__host__ __device__ inline int slots_of(int cls) { return 32 << (3 * (cls - 1)); }

// the class of a row with `key` distinct columns at most (0: nothing to do); `forced` in 1 .. 5 raises it
__host__ __device__ inline int class_of(int key, int forced) {
    if (key <= 0) return 0;
    int c = 1;
    while (c < kSpgemmClasses && key > slots_of(c) / 2) ++c;
    if (forced >= 1 && forced <= kSpgemmClasses && forced > c) c = forced;
    return c;
}

struct MatView {
    const int* rp;
    const int* ci;
    const float* va;
    int rows;
    int limit;        // columns lie in [0, limit)
    long long nnz;
    int ascending;    // columns strictly ascending inside each row
};

__device__ bool matrix_bad(const MatView& M, long long first, long long stride) {
    bool bad = false;
    const long long work = M.nnz > M.rows + 1LL ? M.nnz : (M.rp ? M.rows + 1LL : 0LL);
    for (long long i = first; i < work; i += stride) {
        if (M.rp && i <= M.rows) {
            const int v = M.rp[i];
            if (i == 0 && v != 0) bad = true;
            if (i == M.rows && v != M.nnz) bad = true;
            if (i < M.rows && v > M.rp[i + 1]) bad = true;
        }
        if (i < M.nnz) {
            const int c = M.ci[i];
            if (c < 0 || c >= M.limit) bad = true;
            if (M.ascending && i > 0 && c <= M.ci[i - 1]) {
                // allowed only where entry i starts a row (the search stays inside rp whatever rp holds)
                const int r = upper_bound(M.rp, 0, M.rows + 1, i) - 1;
                if (r < 0 || M.rp[r] != i) bad = true;
            }
        }
    }
    return bad;
}

// one pass over up to three matrices: flags[b] = workgroup b saw a violation
__global__ __launch_bounds__(kThreads) void spgemm_validate_kernel(MatView A, MatView B, MatView C, int with_c,
                                                                   int* __restrict__ flags) {
    const long long first = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    const long long stride = static_cast<long long>(gridDim.x) * kThreads;
    bool bad = matrix_bad(A, first, stride);
    bad = matrix_bad(B, first, stride) || bad;
    if (with_c) bad = matrix_bad(C, first, stride) || bad;
    const int any = __syncthreads_or(bad);
    if (threadIdx.x == 0) flags[blockIdx.x] = any;
}

// block totals of a 64-bit sum and an int maximum, thread 0 writes them
__device__ void block_sum_max(long long sum, int top, long long* __restrict__ part_sum, int* __restrict__ part_max) {
    __shared__ long long s_sum[kThreads / 64];
    __shared__ int s_max[kThreads / 64];
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        top = max(top, __shfl_xor(top, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_max[threadIdx.x >> 6] = top;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            sum += s_sum[w];
            top = max(top, s_max[w]);
        }
        part_sum[blockIdx.x] = sum;
        part_max[blockIdx.x] = top;
    }
}

// work[i] = min(products of row i, INT_MAX); per workgroup the 64-bit total and the largest row.  `lanes` lanes
// share a row of A.
__global__ __launch_bounds__(kThreads) void spgemm_products_kernel(const int* __restrict__ rpA,
                                                                   const int* __restrict__ ciA,
                                                                   const int* __restrict__ rpB, int m, int lanes,
                                                                   int* __restrict__ work,
                                                                   long long* __restrict__ part_sum,
                                                                   int* __restrict__ part_max) {
    const int per = kThreads / lanes;
    const int grp = threadIdx.x / lanes, lane = threadIdx.x % lanes;
    long long sum = 0;
    int top = 0;
    for (long long base = blockIdx.x * static_cast<long long>(per); base < m;
         base += static_cast<long long>(gridDim.x) * per) {
        const long long row = base + grp;
        long long cnt = 0;
        if (row < m) {
            const int a0 = rpA[row], a1 = rpA[row + 1];
            for (int off = lane; off < a1 - a0; off += lanes) {
                const int k = ciA[a0 + off];
                cnt += rpB[k + 1] - rpB[k];
            }
        }
        for (int off = lanes >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, lanes);
        if (row < m && lane == 0) {
            const int clamped = cnt > INT_MAX ? INT_MAX : static_cast<int>(cnt);
            work[row] = clamped;
            sum += cnt;
            top = max(top, clamped);
        }
    }
    block_sum_max(sum, top, part_sum, part_max);
}

// the same totals over an int array (the row counts of the symbolic pass)
__global__ __launch_bounds__(kThreads) void spgemm_totals_kernel(const int* __restrict__ v, int n,
                                                                 long long* __restrict__ part_sum,
                                                                 int* __restrict__ part_max) {
    long long sum = 0;
    int top = 0;
    for (long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kThreads) {
        sum += v[i];
        top = max(top, v[i]);
    }
    block_sum_max(sum, top, part_sum, part_max);
}

// data[c * m + i] = row i belongs to class c, and data[kSegments * m] = 0: an exclusive scan of data then holds
// every row's place in the list of rows by class, and the lists' boundaries.
//   mode 0 (symbolic): key = min(work[i], n)         mode 1 (numeric): key = src[i], the row's distinct count
//   mode 2 (numeric into a given pattern): key = src[i+1] - src[i], C's row length; a row that has products and no
//   entries, or entries and no products, raises the flag
__global__ __launch_bounds__(kThreads) void spgemm_classify_kernel(int mode, const int* __restrict__ src,
                                                                   const int* __restrict__ work, int m, int n,
                                                                   int forced, int* __restrict__ data,
                                                                   int* __restrict__ flags) {
    const long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (i == 0) data[static_cast<long long>(kSegments) * m] = 0;
    if (i >= m) return;
    int key;
    if (mode == 0) key = min(work[i], n);
    else if (mode == 1) key = src[i];
    else {
        key = src[i + 1] - src[i];
        if ((key > 0) != (work[i] > 0)) flags[blockIdx.x % kMaxGrid] = 1;
    }
    const int cls = class_of(key, forced);
#pragma unroll
    for (int c = 0; c < kSegments; ++c) data[static_cast<long long>(c) * m + i] = cls == c;
}

// lists[scan[c * m + i]] = i for the one c row i belongs to; bounds[c] = scan[c * m], c = 0 .. kSegments
__global__ __launch_bounds__(kThreads) void spgemm_lists_kernel(const int* __restrict__ scan, int m,
                                                                int* __restrict__ lists, int* __restrict__ bounds) {
    const long long idx = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    const long long total = static_cast<long long>(kSegments) * m;
    if (idx > total) return;
    if (idx % m == 0) bounds[idx / m] = scan[idx];
    if (idx == total) return;
    if (scan[idx + 1] != scan[idx]) lists[scan[idx]] = static_cast<int>(idx % m);
}

enum Mode { SYMBOLIC = 0, NUMERIC = 1, REFILL = 2 };

// ---- classes 1 .. 4: hash tables in LDS ----------------------------------------------------------------------
// A workgroup holds blockDim.x / gt tables of `slots` slots, each owned by gt consecutive threads that clear, sort
// and write it; the first gl of them (one wavefront's lanes at most) walk the row.  Classes 1 .. 3: gt == gl ==
// lanes; class 4: one table, gt == 256, gl == 64.
// LDS: per table `slots` keys (and `slots` values unless SYMBOLIC), then one claim counter per table.
template <int MODE>
__global__ __launch_bounds__(kThreads) void spgemm_table_kernel(MatView A, MatView B, const int* __restrict__ rows,
                                                                int count, int slots, int gt, int gl,
                                                                int* __restrict__ counts,
                                                                const int* __restrict__ c_rp, int* c_ci, float* c_va,
                                                                int* __restrict__ flags) {
    extern __shared__ int lds[];
    const int tables = blockDim.x / gt;
    const int stride = MODE == SYMBOLIC ? slots : 2 * slots;
    const int grp = threadIdx.x / gt, t = threadIdx.x % gt;
    int* keys = lds + grp * stride;
    float* vals = reinterpret_cast<float*>(keys + slots);       // (not touched when SYMBOLIC)
    int* claimed = lds + tables * stride + grp;
    const int mask = slots - 1;
    bool bad = false;

    for (long long base = blockIdx.x * static_cast<long long>(tables); base < count;
         base += static_cast<long long>(gridDim.x) * tables) {
        const bool have = base + grp < count;
        const int row = have ? rows[base + grp] : 0;
        for (int s = t; s < slots; s += gt) {
            keys[s] = -1;
            if (MODE != SYMBOLIC) vals[s] = 0.0f;
        }
        if (t == 0) *claimed = 0;
        __syncthreads();

        if (have && t < gl) {
            const int a0 = A.rp[row], a1 = A.rp[row + 1];
            for (int p0 = a0; p0 < a1; p0 += min(gl, a1 - p0)) {
                // the group's next gl entries of A and the B rows they point at, one per lane
                int b0 = 0, b1 = 0;
                float av = 0.0f;
                if (t < a1 - p0) {
                    const int k = A.ci[p0 + t];
                    av = A.va ? A.va[p0 + t] : 0.0f;
                    b0 = B.rp[k];
                    b1 = B.rp[k + 1];
                }
                const int steps = min(gl, a1 - p0);
                for (int j = 0; j < steps; ++j) {
                    const int q0 = __shfl(b0, j, gl);
                    const int len = __shfl(b1, j, gl) - q0;
                    const float a = __shfl(av, j, gl);
                    for (int off = t; off < len; off += gl) {
                        const int col = B.ci[q0 + off];
                        int s = col & mask, found = -1;
                        for (int probe = 0; probe < slots; ++probe) {
                            const int prev = atomicCAS(&keys[s], -1, col);
                            if (prev == -1) atomicAdd(claimed, 1);
                            if (prev == -1 || prev == col) {
                                found = s;
                                break;
                            }
                            s = (s + 1) & mask;
                        }
                        if (found < 0) {
                            bad = true;             // table full: only a pattern that does not fit its class
                        } else if (MODE != SYMBOLIC) {
                            // Plain LDS read-modify-write, no atomics: the bits rely on this slot's additions
                            // happening in step order.  That holds because the lanes that walk a row sit in ONE
                            // wavefront, whose LDS accesses complete in program order, and because the lanes
                            // reconverge at the __shfl of the next step before any of them adds again.  Do not
                            // spread the walk of one row over several wavefronts.
                            vals[found] = __fadd_rn(vals[found], __fmul_rn(a, B.va[q0 + off]));
                        }
                    }
                }
            }
        }
        __syncthreads();

        if (MODE == SYMBOLIC) {
            if (have && t == 0) counts[row] = *claimed;
        } else if (MODE == NUMERIC) {
            // bitonic sort of the whole table by key as unsigned: the empty slots (-1) end up last
            for (int k2 = 2; k2 <= slots; k2 <<= 1) {
                for (int j = k2 >> 1; j > 0; j >>= 1) {
                    for (int i = t; i < (slots >> 1); i += gt) {
                        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                        const int hi = lo + j;
                        const unsigned klo = static_cast<unsigned>(keys[lo]), khi = static_cast<unsigned>(keys[hi]);
                        const bool ascending = (lo & k2) == 0;
                        if ((klo > khi) == ascending) {
                            keys[lo] = static_cast<int>(khi);
                            keys[hi] = static_cast<int>(klo);
                            const float v = vals[lo];
                            vals[lo] = vals[hi];
                            vals[hi] = v;
                        }
                    }
                    __syncthreads();
                }
            }
            if (have) {
                const int out = c_rp[row], len = c_rp[row + 1] - out;
                if (*claimed != len) bad = true;
                const int n_out = min(len, *claimed);
                for (int j = t; j < n_out; j += gt) {
                    c_ci[out + j] = keys[j];
                    c_va[out + j] = vals[j];
                }
            }
        } else {
            if (have) {
                const int out = c_rp[row], len = c_rp[row + 1] - out;
                if (*claimed != len) bad = true;
                for (int j = t; j < len; j += gt) {
                    const int col = c_ci[out + j];
                    int s = col & mask, found = -1;
                    for (int probe = 0; probe < slots; ++probe) {
                        const int k = keys[s];
                        if (k == col) found = s;
                        if (k == col || k == -1) break;
                        s = (s + 1) & mask;
                    }
                    if (found < 0) bad = true; else c_va[out + j] = vals[found];
                }
            }
        }
        __syncthreads();
    }
    const int any = __syncthreads_or(bad);
    if (any && threadIdx.x == 0) flags[blockIdx.x] = 1;
}

// ---- the dense class -----------------------------------------------------------------------------------------
__device__ __forceinline__ int block_sum(int v, int* s_wave) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                    // (s_wave may still be read from the call before)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// One workgroup per row at a time; its slice of scratch is n floats (not when SYMBOLIC) and an n-bit map, all zero
// between rows.  The first wavefront walks the row; all four write it out and clear what it touched.
template <int MODE>
__global__ __launch_bounds__(kThreads) void spgemm_dense_kernel(MatView A, MatView B, const int* __restrict__ rows,
                                                                int count, int n, float* acc_all, unsigned* map_all,
                                                                int* __restrict__ counts,
                                                                const int* __restrict__ c_rp, int* c_ci, float* c_va,
                                                                int* __restrict__ flags) {
    __shared__ int s_wave[kThreads / 64];
    const long long words = (static_cast<long long>(n) + 31) >> 5;
    float* acc = MODE == SYMBOLIC ? nullptr : acc_all + blockIdx.x * static_cast<size_t>(n);
    unsigned* map = map_all + blockIdx.x * static_cast<size_t>(words);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad = false;

    for (long long idx = blockIdx.x; idx < count; idx += gridDim.x) {
        const int row = rows[idx];
        if (wave == 0) {
            const int a0 = A.rp[row], a1 = A.rp[row + 1];
            for (int p0 = a0; p0 < a1; p0 += min(64, a1 - p0)) {
                int b0 = 0, b1 = 0;
                float av = 0.0f;
                if (lane < a1 - p0) {
                    const int k = A.ci[p0 + lane];
                    av = A.va ? A.va[p0 + lane] : 0.0f;
                    b0 = B.rp[k];
                    b1 = B.rp[k + 1];
                }
                const int steps = min(64, a1 - p0);
                for (int j = 0; j < steps; ++j) {
                    const int q0 = __shfl(b0, j, 64);
                    const int len = __shfl(b1, j, 64) - q0;
                    const float a = __shfl(av, j, 64);
                    for (int off0 = 0; off0 < len; off0 += 64) {        // (uniform: every lane takes the shuffles)
                        const bool active = lane < len - off0;
                        int col = 0;
                        if (active) {
                            col = B.ci[q0 + off0 + lane];
                            // acc[] and map[] are plain global memory: the order of a column's additions (and of
                            // the ORs into a map word) is the program order of this one wavefront, the only one
                            // that touches the slice until the barrier below.  Keep the walk in one wavefront.
                            if (MODE != SYMBOLIC) acc[col] = __fadd_rn(acc[col], __fmul_rn(a, B.va[q0 + off0 + lane]));
                        }
                        // the columns ascend from lane to lane, so the lanes of one map word are neighbours: OR their
                        // bits together (a segmented scan) and let the last lane of the word store it
                        const int word = active ? col >> 5 : -1;
                        unsigned bits = active ? 1u << (col & 31) : 0u;
#pragma unroll
                        for (int d = 1; d < 64; d <<= 1) {
                            const int other_word = __shfl_up(word, d, 64);
                            const unsigned other_bits = __shfl_up(bits, d, 64);
                            if (lane >= d && other_word == word) bits |= other_bits;
                        }
                        const int next_word = __shfl_down(word, 1, 64);
                        if (active && (lane == 63 || next_word != word)) map[word] |= bits;
                    }
                }
            }
        }
        __syncthreads();

        const int out = MODE == SYMBOLIC ? 0 : c_rp[row];
        const int len = MODE == SYMBOLIC ? 0 : c_rp[row + 1] - out;
        if (MODE == REFILL) {
            // every stored column must have been produced, and there must be as many as were produced
            int mine = 0;
            for (long long w = threadIdx.x; w < words; w += kThreads) mine += __popc(map[w]);
            if (block_sum(mine, s_wave) != len) bad = true;
            for (int j = threadIdx.x; j < len; j += kThreads) {
                const int col = c_ci[out + j];
                if ((map[col >> 5] >> (col & 31)) & 1u) c_va[out + j] = acc[col]; else bad = true;
            }
            __syncthreads();
        }
        int run = 0;
        for (long long w0 = 0; w0 < words; w0 += kThreads) {
            const long long w = w0 + threadIdx.x;
            unsigned bits = w < words ? map[w] : 0u;
            const int pc = __popc(bits);
            if (MODE == NUMERIC) {
                const int incl = dev::wave_inclusive_scan(pc);
                __syncthreads();
                if (lane == 63) s_wave[wave] = incl;
                __syncthreads();
                int before = 0, total = 0;
                for (int v = 0; v < kThreads / 64; ++v) {
                    if (v < wave) before += s_wave[v];
                    total += s_wave[v];
                }
                int pos = run + before + incl - pc;
                run += total;
                if (pos + pc > len) {
                    bad = true;                      // more columns than the row pointers promise: write none
                } else {
                    for (unsigned left = bits; left; left &= left - 1) {
                        const int col = static_cast<int>(w << 5) + __ffs(left) - 1;
                        c_ci[out + pos] = col;
                        c_va[out + pos] = acc[col];
                        ++pos;
                    }
                }
            } else {
                run += pc;
            }
            if (pc) {
                if (MODE != SYMBOLIC) {
                    for (unsigned left = bits; left; left &= left - 1) {
                        acc[(w << 5) + __ffs(left) - 1] = 0.0f;
                    }
                }
                map[w] = 0u;
            }
        }
        if (MODE == SYMBOLIC) {
            const int total = block_sum(run, s_wave);
            if (threadIdx.x == 0) counts[row] = total;
        } else if (MODE == NUMERIC) {
            if (run != len) bad = true;
        }
        __syncthreads();
    }
    const int any = __syncthreads_or(bad);
    if (any && threadIdx.x == 0) flags[blockIdx.x] = 1;
}

// ---- host side -----------------------------------------------------------------------------------------------
bool good(hipError_t e) { return e == hipSuccess; }

unsigned blocks_for(long long n, long long per) { return static_cast<unsigned>((n + per - 1) / per); }

struct Scratch {
    std::vector<void*> held;
    template <typename T>
    bool get(T** p, size_t count) {
        *p = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
            *p = nullptr;
            (void)hipGetLastError();
            return false;
        }
        held.push_back(*p);
        return true;
    }
    ~Scratch() {
        for (void* p : held) (void)hipFree(p);
    }
};

MatView view_of(const CSRMatrix* M, int limit, bool ascending) {
    return MatView{M->d_row_ptrs, M->d_col_indices, M->d_values, M->num_rows, limit, M->nnz, ascending ? 1 : 0};
}

int lanes_for(const CSRMatrix* B) {
    if (int f = forced_lanes("spgemm_lanes")) return f;
    return pick_lanes_per_row(static_cast<float>(B->nnz) / static_cast<float>(std::max(B->num_rows, 1)));
}

// everything one call holds on the device besides C
struct Job {
    hipStream_t s;
    MatView A, B;
    int m, n, lanes, forced;
    int* work = nullptr;        // [m] products per row, clamped
    int* data = nullptr;        // [kSegments * m + 1] class flags, then their scan; the scan's sums behind it
    int* lists = nullptr;       // [m] rows by class
    int* bounds = nullptr;      // [kSegments + 1]
    int* flags = nullptr;       // [kMaxGrid]
    long long* part_sum = nullptr;   // [kMaxGrid]
    int* part_max = nullptr;         // [kMaxGrid]
    std::vector<long long> levels;
    int host_bounds[kSegments + 1] = {};
};

bool job_alloc(Job& job, Scratch& scratch) {
    job.levels = device_scan_levels(static_cast<long long>(kSegments) * job.m + 1);
    return scratch.get(&job.work, job.m) && scratch.get(&job.data, job.levels[0] + device_scan_sums(job.levels)) &&
           scratch.get(&job.lists, job.m) && scratch.get(&job.bounds, kSegments + 1) &&
           scratch.get(&job.flags, kMaxGrid) && scratch.get(&job.part_sum, kMaxGrid) &&
           scratch.get(&job.part_max, kMaxGrid) &&
           hipMemsetAsync(job.flags, 0, sizeof(int) * kMaxGrid, job.s) == hipSuccess;
}

// reads the per-workgroup totals of the launch before (synchronises)
bool read_totals(Job& job, unsigned grid, long long* sum, int* top) {
    std::vector<long long> sums(grid);
    std::vector<int> tops(grid);
    if (hipMemcpyAsync(sums.data(), job.part_sum, grid * sizeof(long long), hipMemcpyDeviceToHost, job.s) != hipSuccess ||
        hipMemcpyAsync(tops.data(), job.part_max, grid * sizeof(int), hipMemcpyDeviceToHost, job.s) != hipSuccess ||
        hipStreamSynchronize(job.s) != hipSuccess) {
        return false;
    }
    *sum = 0;
    *top = 0;
    for (unsigned b = 0; b < grid; ++b) {
        *sum += sums[b];
        *top = std::max(*top, tops[b]);
    }
    return true;
}

// the lists of rows by class for `mode` (spgemm_classify_kernel); bounds stay on the device until read_bounds
hipError_t enqueue_lists(Job& job, int mode, const int* src) {
    const int m = job.m;
    spgemm_classify_kernel<<<blocks_for(m, kThreads), kThreads, 0, job.s>>>(mode, src, job.work, m, job.n, job.forced,
                                                                           job.data, job.flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = device_exclusive_scan(job.data, job.levels, job.data + job.levels[0], job.s);
    if (e != hipSuccess) return e;
    spgemm_lists_kernel<<<blocks_for(job.levels[0], kThreads), kThreads, 0, job.s>>>(job.data, m, job.lists, job.bounds);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(job.host_bounds, job.bounds, sizeof(job.host_bounds), hipMemcpyDeviceToHost, job.s);
}

template <int MODE>
hipError_t launch_tables(Job& job, int cls, int first, int count, int* counts, const int* c_rp, int* c_ci,
                         float* c_va) {
    const int slots = slots_of(cls);
    const int table_bytes = slots * (MODE == SYMBOLIC ? 4 : 8);
    int gt = job.lanes, gl = job.lanes, tables = std::max(1, std::min(kThreads / job.lanes, kTableBudget / table_bytes));
    if (cls == kSpgemmClasses - 1) {        // the largest table: one per workgroup, a whole wavefront walks the row
        gt = kThreads;
        gl = 64;
        tables = 1;
    }
    const size_t lds = static_cast<size_t>(tables) * table_bytes + sizeof(int) * tables;
    const void* kernel = reinterpret_cast<const void*>(&spgemm_table_kernel<MODE>);
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    const unsigned grid = std::min<unsigned>(kMaxGrid, blocks_for(count, tables));
    spgemm_table_kernel<MODE><<<grid, tables * gt, lds, job.s>>>(job.A, job.B, job.lists + first, count, slots, gt, gl,
                                                                 counts, c_rp, c_ci, c_va, job.flags);
    return hipGetLastError();
}

int dense_groups(int n, int count, bool symbolic) {
    const long long words = (static_cast<long long>(n) + 31) >> 5;
    const long long slice = words * 4 + (symbolic ? 0LL : 4LL * n);
    long long groups = std::max(1LL, std::min<long long>(kThreads, kDenseScratchCap / std::max(slice, 1LL)));
    long long forced = 0;
    if (debug_option("spgemm_dense_groups", &forced) && forced >= 1) groups = std::min<long long>(forced, kMaxGrid);
    return static_cast<int>(std::min<long long>(groups, count));
}

template <int MODE>
hipError_t launch_dense(Job& job, Scratch& scratch, int first, int count, int* counts, const int* c_rp, int* c_ci,
                        float* c_va, bool* out_of_memory) {
    const int groups = dense_groups(job.n, count, MODE == SYMBOLIC);
    const size_t words = static_cast<size_t>((static_cast<long long>(job.n) + 31) >> 5);
    float* acc = nullptr;
    unsigned* map = nullptr;
    if (!scratch.get(&map, words * groups) || (MODE != SYMBOLIC && !scratch.get(&acc, static_cast<size_t>(job.n) * groups))) {
        *out_of_memory = true;
        return hipErrorOutOfMemory;
    }
    hipError_t e = hipMemsetAsync(map, 0, words * groups * sizeof(unsigned), job.s);
    if (e == hipSuccess && acc) e = hipMemsetAsync(acc, 0, static_cast<size_t>(job.n) * groups * sizeof(float), job.s);
    if (e != hipSuccess) return e;
    spgemm_dense_kernel<MODE><<<groups, kThreads, 0, job.s>>>(job.A, job.B, job.lists + first, count, job.n, acc, map,
                                                              counts, c_rp, c_ci, c_va, job.flags);
    return hipGetLastError();
}

// one pass over the rows of classes 1 .. kSpgemmClasses, from the bounds read_bounds left in job.host_bounds
template <int MODE>
hipError_t launch_pass(Job& job, Scratch& scratch, int* counts, const int* c_rp, int* c_ci, float* c_va,
                       bool* out_of_memory) {
    for (int cls = 1; cls <= kSpgemmClasses; ++cls) {
        const int first = job.host_bounds[cls], count = job.host_bounds[cls + 1] - first;
        if (count <= 0) continue;
        const hipError_t e = cls < kSpgemmClasses
            ? launch_tables<MODE>(job, cls, first, count, counts, c_rp, c_ci, c_va)
            : launch_dense<MODE>(job, scratch, first, count, counts, c_rp, c_ci, c_va, out_of_memory);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void histogram(const Job& job, int* out) {
    for (int c = 0; c < kSegments; ++c) out[c] = job.host_bounds[c + 1] - job.host_bounds[c];
}

// true when some workgroup raised its flag (synchronises); *ok = false when the read itself failed
bool any_flag(Job& job, bool* ok) {
    std::vector<int> flags(kMaxGrid);
    *ok = hipMemcpyAsync(flags.data(), job.flags, sizeof(int) * kMaxGrid, hipMemcpyDeviceToHost, job.s) == hipSuccess &&
          hipStreamSynchronize(job.s) == hipSuccess;
    for (int f : flags) if (f) return true;
    return false;
}

// check 5: the one validation launch, read before anything else is allocated
int validate(const CSRMatrix* A, const CSRMatrix* B, const CSRMatrix* C, hipStream_t s) {
    const MatView a = view_of(A, B->num_rows, false), b = view_of(B, B->num_cols, true);
    const MatView c = C ? view_of(C, C->num_cols, false) : MatView{};
    long long work = std::max({a.nnz, b.nnz, c.nnz, a.rows + 1LL, b.rows + 1LL, c.rows + 1LL});
    const unsigned grid = std::min<unsigned>(2048, std::max(1u, blocks_for(work, kThreads)));
    int* d_flags = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d_flags), sizeof(int) * grid) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    std::vector<int> flags(grid);
    spgemm_validate_kernel<<<grid, kThreads, 0, s>>>(a, b, c, C ? 1 : 0, d_flags);
    const bool ok = hipGetLastError() == hipSuccess &&
                    hipMemcpyAsync(flags.data(), d_flags, grid * sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess;
    (void)hipFree(d_flags);
    if (!ok) return code(SpMVError::KERNEL_LAUNCH);
    for (int f : flags) if (f) return code(SpMVError::INVALID_FORMAT);
    return code(SpMVError::SUCCESS);
}

// checks 1 - 5 of spgemm.h, then the products per row: what both entry points start with
int begin(Job& job, Scratch& scratch, const CSRMatrix* C, bool refill, const CSRMatrix* A, const CSRMatrix* B,
          SpGEMMResult* result, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!C || !A || !B) return fail(result, SpMVError::INVALID_ARGUMENT);
    if (C == A || C == B) return fail(result, SpMVError::INVALID_ARGUMENT);
    if (A->num_cols != B->num_rows) return fail(result, SpMVError::INVALID_DIMENSION);
    if (refill && (C->num_rows != A->num_rows || C->num_cols != B->num_cols)) {
        return fail(result, SpMVError::INVALID_DIMENSION);
    }
    if (!device_arrays_lenient(A) || !device_arrays_lenient(B) || (refill && !device_arrays_lenient(C))) {
        return fail(result, SpMVError::INVALID_FORMAT);
    }
    const int status = validate(A, B, refill ? C : nullptr, job.s);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));

    job.A = view_of(A, B->num_rows, false);
    job.B = view_of(B, B->num_cols, true);
    job.m = A->num_rows;
    job.n = B->num_cols;
    job.lanes = lanes_for(B);
    job.forced = static_cast<int>(debug_number("spgemm_class", 0));
    result->lanes = job.lanes;
    if (job.m == 0 || job.n == 0 || A->nnz == 0 || B->nnz == 0) {
        result->symbolic_rows[0] = result->numeric_rows[0] = job.m;
        *nothing_to_do = true;
        return 0;
    }
    if (!job_alloc(job, scratch)) return fail(result, SpMVError::CUDA_MALLOC);
    const int a_lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / static_cast<float>(job.m));
    const unsigned grid = std::min<unsigned>(kMaxGrid, blocks_for(job.m, kThreads / a_lanes));
    spgemm_products_kernel<<<grid, kThreads, 0, job.s>>>(job.A.rp, job.A.ci, job.B.rp, job.m, a_lanes, job.work,
                                                         job.part_sum, job.part_max);
    if (!good(hipGetLastError()) || !read_totals(job, grid, &result->products, &result->max_row_products)) {
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    if (result->products == 0) {
        result->symbolic_rows[0] = result->numeric_rows[0] = job.m;
        *nothing_to_do = true;
    }
    return 0;
}

} // namespace

int spgemm_build(const CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, DeviceCsrArrays* out, int* out_nnz,
                 SpGEMMResult* result, hipStream_t s) {
    *out = DeviceCsrArrays();
    *out_nnz = 0;
    *result = SpGEMMResult();
    Scratch scratch;
    Job job;
    job.s = s;
    bool nothing = false;
    if (begin(job, scratch, C, false, A, B, result, &nothing) != 0) return result->error_code;
    const TraceRange range("spmv:spgemm_csr");
    const int m = A->num_rows;

    DeviceCsrArrays c;
    if (c.alloc(static_cast<long long>(m) + 1, 0) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    bool ok = hipMemsetAsync(c.row_ptrs, 0, (static_cast<size_t>(m) + 1) * sizeof(int), s) == hipSuccess;
    if (nothing) {
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) {
            c.release();
            return fail(result, SpMVError::KERNEL_LAUNCH);
        }
        *out = c;
        return 0;
    }

    Events ev;
    bool oom = false;
    // ---- symbolic: counts into c.row_ptrs, their totals, the numeric lists, then the scan into row pointers ----
    ok = ok && ev.ok && hipEventRecord(ev.e[0], s) == hipSuccess;
    ok = ok && good(enqueue_lists(job, 0, nullptr)) && good(hipStreamSynchronize(s));
    if (ok) histogram(job, result->symbolic_rows);
    ok = ok && good(launch_pass<SYMBOLIC>(job, scratch, c.row_ptrs, nullptr, nullptr, nullptr, &oom));
    const unsigned grid = std::min<unsigned>(kMaxGrid, blocks_for(m, kThreads));
    long long nnz = 0;
    if (ok) {
        spgemm_totals_kernel<<<grid, kThreads, 0, s>>>(c.row_ptrs, m, job.part_sum, job.part_max);
        ok = good(hipGetLastError()) && good(enqueue_lists(job, 1, c.row_ptrs));
    }
    if (ok) {
        const std::vector<long long> levels = device_scan_levels(static_cast<long long>(m) + 1);
        // (job.data is free again once the lists are out: the row-pointer scan borrows its head for the sums)
        ok = good(device_exclusive_scan(c.row_ptrs, levels, job.data, s)) &&
             hipEventRecord(ev.e[1], s) == hipSuccess && read_totals(job, grid, &nnz, &result->max_row_nnz);
    }
    bool flagged = false;
    if (ok) flagged = any_flag(job, &ok); else (void)hipStreamSynchronize(s);
    if (!ok || flagged) {
        c.release();
        return fail(result, oom ? SpMVError::CUDA_MALLOC : SpMVError::KERNEL_LAUNCH);
    }
    histogram(job, result->numeric_rows);
    if (nnz > INT_MAX) {
        c.release();
        return fail(result, SpMVError::INVALID_DIMENSION);
    }
    (void)hipEventElapsedTime(&result->symbolic_ms, ev.e[0], ev.e[1]);

    // ---- numeric ----
    if (c.alloc_entries(nnz) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    ok = hipEventRecord(ev.e[2], s) == hipSuccess &&
         good(launch_pass<NUMERIC>(job, scratch, nullptr, c.row_ptrs, c.col_indices, c.values, &oom)) &&
         hipEventRecord(ev.e[3], s) == hipSuccess;
    if (ok) flagged = any_flag(job, &ok); else (void)hipStreamSynchronize(s);
    if (!ok || flagged) {
        c.release();
        return fail(result, oom ? SpMVError::CUDA_MALLOC : SpMVError::KERNEL_LAUNCH);
    }
    (void)hipEventElapsedTime(&result->numeric_ms, ev.e[2], ev.e[3]);
    result->nnz = static_cast<int>(nnz);
    *out_nnz = static_cast<int>(nnz);
    *out = c;
    return 0;
}

int spgemm_refill(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, SpGEMMResult* result, hipStream_t s) {
    *result = SpGEMMResult();
    Scratch scratch;
    Job job;
    job.s = s;
    bool nothing = false;
    if (begin(job, scratch, C, true, A, B, result, &nothing) != 0) return result->error_code;
    const TraceRange range("spmv:spgemm_csr_numeric");
    result->nnz = C->nnz;
    if (nothing) return C->nnz == 0 ? 0 : fail(result, SpMVError::INVALID_FORMAT);

    Events ev;
    bool oom = false;
    bool ok = ev.ok && enqueue_lists(job, 2, C->d_row_ptrs) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
    if (ok) histogram(job, result->numeric_rows);
    ok = ok && hipEventRecord(ev.e[2], s) == hipSuccess &&
         launch_pass<REFILL>(job, scratch, nullptr, C->d_row_ptrs, C->d_col_indices, C->d_values, &oom) == hipSuccess &&
         hipEventRecord(ev.e[3], s) == hipSuccess;
    bool flagged = false;
    if (ok) flagged = any_flag(job, &ok); else (void)hipStreamSynchronize(s);
    if (!ok) return fail(result, oom ? SpMVError::CUDA_MALLOC : SpMVError::KERNEL_LAUNCH);
    if (flagged) return fail(result, SpMVError::INVALID_FORMAT);
    (void)hipEventElapsedTime(&result->numeric_ms, ev.e[2], ev.e[3]);
    return 0;
}

} // namespace detail

int spgemm_csr(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, SpGEMMResult* result) {
    SpGEMMResult local;
    SpGEMMResult* r = result ? result : &local;
    detail::DeviceCsrArrays c;
    const detail::ReleaseOnExit release_c{&c};
    int nnz = 0;
    const int status = detail::spgemm_build(C, A, B, &c, &nnz, r, detail::current_stream());
    if (status != 0) return status;
    detail::csr_adopt_device(C, A->num_rows, B->num_cols, nnz, &c);
    return 0;
}

int spgemm_csr_numeric(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, SpGEMMResult* result) {
    SpGEMMResult local;
    return detail::spgemm_refill(C, A, B, result ? result : &local, detail::current_stream());
}

} // namespace spmv
