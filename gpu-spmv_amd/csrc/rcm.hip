// rcm.hip — reverse Cuthill-McKee on the device and the band statistics (include/spmv/reorder.h).
//
//   csr_rcm   S = the pattern of A + A^T (A itself when the caller promises symmetry), D = the vertices by (degree,
//             index) from the stable counting sort of color_ordering, S' = D S D^T from csr_permute_gpu.  In S' the
//             smallest key is the smallest index and every row lists its neighbours in key order, so nothing in the
//             loop sorts.  A level structure is numbered level by level, in queue order:
//               parents   every vertex u of the level, at position p, offers p to each unvisited neighbour with an
//                         integer atomicMin: the neighbour's parent is the earliest position that stores it, whatever
//                         order the offers arrive in.  The offers carry the sweep's epoch in their high word, so no
//                         array is cleared between sweeps.
//               counts    u counts the entries of its row whose parent is p; an exclusive scan of the counts in
//                         position order gives every parent its slice of the next level.
//               children  the entry's rank among u's children is the number of children to its left in the row (a
//                         ballot and a popcount over the row's lanes, carried over the row's steps); it is stored at
//                         slice + rank, compared with n first.
//             A run of levels of at most 256 vertices is one launch of one workgroup (rcm_run_kernel, barriers between
//             the passes); a wider level takes four launches (parents, counts, the scan of the per-chunk totals,
//             children).  The run kernel also closes a sweep and opens the next: the George-Liu search is decided on
//             the device, and the host only reads a small state after every batch of rounds.
//   csr_band  one pass, LANES lanes per row, a per-workgroup max and 64-bit sum, then a one-workgroup fold.
// No kernel here waits for another workgroup.  The only atomics on data are the integer minima above.
#include "rcm_impl.h"
#include "solver_common.h"
#include "spmv/csr_ops.h"

#include <climits>
#include <vector>

namespace spmv {
namespace detail {
namespace rcm {

namespace {

using dev::capped_grid;
using dev::kBlock;
using dev::vec_grid;
using dev::wave_inclusive_scan;
using dev::with_lanes;

constexpr int kNumbered = INT_MAX;      // mark[v]: numbered for good (0: never seen, e >= 1: seen by sweep e)
enum Phase { FIRST = 0, TRY = 1, FINAL = 2 };

// the device state of one ordering
struct RcmState {
    int start, width;            // the level to number next: queue[start, start + width)
    int next_start, next_width;  // written by the wide scan, taken over by the next run launch when `pending`
    int pending;
    int open;                    // a sweep is in progress
    int started;
    int closed_final;            // the sweep that closed last numbered its component for good
    int comp_start;              // vertices numbered by the components done so far
    int tail;                    // end of the closed sweep's slice of the queue
    int height;                  // levels of the sweep so far
    int phase;
    int final_sweep;             // this sweep's marks are for good
    int epoch;
    int root, best_root, best_height, last_min;
    int cursor;                  // every index below it is numbered
    int isolated;                // vertices of degree 0: the indices below it
    int components, levels, sweeps;
    int progress;                // sweeps opened and closed + levels numbered: the host's proof that a batch moved
    int error;                   // a position past the queue's end: a broken invariant
    int finished;
};

__device__ __forceinline__ int peek(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void poke(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long peek(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the offer of position p in sweep `epoch`: a later sweep's offers are smaller than anything an earlier one left
__device__ __forceinline__ unsigned long long offer(int epoch, int p) {
    return (static_cast<unsigned long long>(0xffffffffu - static_cast<unsigned>(epoch)) << 32) | static_cast<unsigned>(p);
}

// ---- the three passes over one row, shared by the run kernel and the wide kernels ----
// pass 1: the row of the vertex at position p offers p to every neighbour this sweep has not seen
template <int LANES>
__device__ __forceinline__ void offer_row(int begin, int end, int lane, int epoch, int p, const int* __restrict__ ci,
                                          const int* mark, unsigned long long* pkey) {
    const unsigned long long mine = offer(epoch, p);
    for (int j = begin + lane; j < end; j += LANES) {
        const int x = ci[j];
        const int m = peek(&mark[x]);
        if (m != epoch && m != kNumbered) atomicMin(&pkey[x], mine);
    }
}

// passes 2 and 3: walks the row in steps of LANES entries; child(rank, x) is called for every entry x whose parent is
// p, with the number of such entries to its left.  Returns their count, in every lane of the row.  Called by whole
// wavefronts (`active` = this group has a row); the trip count is the wavefront's longest row.
template <int LANES, class Child>
__device__ __forceinline__ int walk_children(bool active, int begin, int end, int lane, int epoch, int p,
                                             const int* __restrict__ ci, const unsigned long long* pkey,
                                             Child&& child) {
    const unsigned long long mine = offer(epoch, p);
    const int lane_in_wave = threadIdx.x & 63;
    const unsigned long long group =
        LANES == 64 ? ~0ull : ((1ull << (LANES & 63)) - 1ull) << (lane_in_wave - lane);      // the row's lanes
    const unsigned long long below = (1ull << lane_in_wave) - 1ull;
    int carry = 0;
    for (int base = begin;; base += LANES) {
        const int j = base + lane;
        const bool in = active && j < end;
        if (!__any(in)) break;
        const int x = in ? ci[j] : 0;
        const bool is_child = in && peek(&pkey[x]) == mine;
        const unsigned long long votes = __ballot(is_child) & group;
        if (is_child) child(carry + __popcll(votes & below), x);
        carry += __popcll(votes);
    }
    return carry;
}

// s_off[t] = the exclusive prefix sum of s_cnt[t] over the kBlock slots; returns the total.  Called by the whole
// workgroup; s_wave: kBlock / 64 ints.  Ends with a barrier.
__device__ __forceinline__ int block_exclusive_scan(const int* s_cnt, int* s_off, int* s_wave) {
    const int v = s_cnt[threadIdx.x];
    const int inc = wave_inclusive_scan(v);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < static_cast<int>(threadIdx.x >> 6)) before += s_wave[w];
        total += s_wave[w];
    }
    s_off[threadIdx.x] = before + inc - v;
    __syncthreads();
    return total;
}

// the smallest of the workgroup's values in every thread; s_wave: kBlock / 64 ints.  Barriers before and after.
__device__ __forceinline__ int block_min_all(int v, int* s_wave) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = s_wave[0];
    for (int w = 1; w < kBlock / 64; ++w) m = min(m, s_wave[w]);
    __syncthreads();
    return m;
}

// A sweep's last level has been numbered and has no children: what the search does next.  One thread.
__device__ void close_sweep(RcmState* st, int peripheral, int last_min) {
    ++st->sweeps;
    ++st->progress;
    st->tail = st->start + st->width;
    st->last_min = last_min;
    bool final = false;
    if (st->phase == FIRST) {
        st->best_root = st->root;
        st->best_height = st->height;
        if (peripheral) {
            st->phase = TRY;
            st->root = last_min;
        } else {
            final = true;
        }
    } else if (st->phase == TRY) {
        if (st->height > st->best_height) {                       // a taller structure: search on from its far end
            st->best_root = st->root;
            st->best_height = st->height;
            st->root = last_min;
        } else {
            st->root = st->best_root;
            st->phase = FINAL;
        }
    } else {
        final = true;
    }
    if (final) {
        ++st->components;
        st->levels += st->height;
    }
    st->closed_final = final ? 1 : 0;
    st->open = 0;
}

// ---- set-up ----
// The isolated vertices are the indices below state->isolated (S' is ordered by degree): numbered here, each a
// component of one level.  degree: by S' index.
__global__ __launch_bounds__(kBlock) void rcm_init_kernel(int n, const int* __restrict__ degree,
                                                          const int* __restrict__ by_key, int* __restrict__ queue,
                                                          int* __restrict__ mark, RcmState* __restrict__ state) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const bool lone = degree[by_key[i]] == 0;
        if (lone) {
            queue[i] = static_cast<int>(i);
            mark[i] = kNumbered;
            if (i + 1 == n || degree[by_key[i + 1]] != 0) state->isolated = static_cast<int>(i) + 1;
        }
    }
}

// columns strictly ascending inside every row of a structure that passed structure_checked
__global__ __launch_bounds__(kBlock) void rcm_ascending_kernel(int n, const int* __restrict__ rp,
                                                               const int* __restrict__ ci, int* __restrict__ flag) {
    bool bad = false;
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        for (int j = rp[i] + 1; j < rp[i + 1]; ++j) bad = bad || ci[j] <= ci[j - 1];
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *flag = 1;
}

// degree[v] = row v's entries other than (v, v); rows are strictly ascending
__global__ __launch_bounds__(kBlock) void rcm_degree_kernel(int n, const int* __restrict__ rp,
                                                            const int* __restrict__ ci, int* __restrict__ degree) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int begin = rp[i], end = rp[i + 1];
        degree[i] = end - begin - (dev::find_column(ci, begin, end, static_cast<int>(i)) >= 0 ? 1 : 0);
    }
}

// ---- the run kernel: one workgroup ----
// Takes over a pending wide level, opens a sweep when none is open (the next root is the lowest index not numbered),
// then numbers levels for as long as they are narrow, up to kRunLevels of them, and closes the sweep when a level has
// no children.
template <int LANES>
__global__ __launch_bounds__(kBlock)
void rcm_run_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, int* queue, int* mark,
                    unsigned long long* pkey, RcmState* state, int peripheral) {
    constexpr int kRows = kBlock / LANES;
    __shared__ int s_cnt[kBlock];
    __shared__ int s_off[kBlock];
    __shared__ int s_wave[kBlock / 64];
    __shared__ int s_go;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;

    if (threadIdx.x == 0) {
        if (state->pending) {
            state->start = state->next_start;
            state->width = state->next_width;
            state->pending = 0;
        }
        int go = (state->finished || state->error) ? 0 : 1;
        if (go && !state->open) {
            if (!state->started) {
                state->started = 1;
                state->comp_start = state->components = state->levels = state->cursor = state->isolated;
                state->closed_final = 1;
            } else if (state->closed_final) {
                state->comp_start = state->tail;
            }
            if (state->comp_start >= n) {
                state->finished = 1;
                go = 0;
            } else {
                go = 2;                                           // a sweep to open
            }
        }
        s_go = go;
    }
    __syncthreads();
    const int go = s_go;
    if (go == 0) return;
    if (go == 2) {
        if (state->closed_final) {                                // a new component: its root is the smallest key left
            int cursor = state->cursor;
            int found = INT_MAX;
            while (cursor < n) {
                const int i = cursor + static_cast<int>(threadIdx.x);
                found = block_min_all(i < n && peek(&mark[i]) != kNumbered ? i : INT_MAX, s_wave);
                if (found != INT_MAX) break;
                cursor += kBlock;
            }
            if (threadIdx.x == 0) {
                if (found == INT_MAX) {
                    state->error = 1;                             // vertices are left and none was found
                } else {
                    state->cursor = found;
                    state->root = found;
                    state->phase = FIRST;
                }
            }
        }
        if (threadIdx.x == 0 && !state->error) {
            const int at = state->comp_start;
            state->epoch += 1;
            state->final_sweep = (state->phase == FINAL || !peripheral) ? 1 : 0;
            poke(&queue[at], state->root);
            poke(&mark[state->root], state->final_sweep ? kNumbered : state->epoch);
            state->start = at;
            state->width = 1;
            state->height = 1;
            state->open = 1;
            ++state->progress;
        }
        __syncthreads();
        if (state->error) return;
    }

    const int epoch = state->epoch;
    const int stamp = state->final_sweep ? kNumbered : epoch;
    int start = state->start, width = state->width;
    for (int done = 0; done < kRunLevels && width <= kNarrow; ++done) {
        // parents
        for (int r = slot; r < width; r += kRows) {
            const int u = peek(&queue[start + r]);
            offer_row<LANES>(rp[u], rp[u + 1], lane, epoch, start + r, ci, mark, pkey);
        }
        __syncthreads();
        // counts
        s_cnt[threadIdx.x] = 0;
        __syncthreads();
        for (int first = 0; first < width; first += kRows) {
            const int r = first + slot;
            const bool active = r < width;
            const int u = active ? peek(&queue[start + r]) : 0;
            const int count = walk_children<LANES>(active, active ? rp[u] : 0, active ? rp[u + 1] : 0, lane, epoch,
                                                   start + r, ci, pkey, [](int, int) {});
            if (active && lane == 0) s_cnt[r] = count;
        }
        __syncthreads();
        const int total = block_exclusive_scan(s_cnt, s_off, s_wave);
        const int next = start + width;
        if (total > n - next) {                                   // more children than vertices left
            if (threadIdx.x == 0) state->error = 1;
            return;
        }
        // children
        for (int first = 0; first < width; first += kRows) {
            const int r = first + slot;
            const bool active = r < width;
            const int u = active ? peek(&queue[start + r]) : 0;
            const int slice = next + (active ? s_off[r] : 0);
            walk_children<LANES>(active, active ? rp[u] : 0, active ? rp[u + 1] : 0, lane, epoch, start + r, ci, pkey,
                                 [&](int rank, int x) {
                                     const int at = slice + rank;
                                     if (at >= 0 && at < n) {
                                         poke(&queue[at], x);
                                         poke(&mark[x], stamp);
                                     }
                                 });
        }
        __syncthreads();
        if (total == 0) {
            const int t = threadIdx.x;
            const int last_min = block_min_all(t < width ? peek(&queue[start + t]) : INT_MAX, s_wave);
            if (threadIdx.x == 0) {
                state->start = start;
                state->width = width;
                close_sweep(state, peripheral, last_min);
            }
            return;
        }
        start = next;
        width = total;
        if (threadIdx.x == 0) {
            state->start = start;
            state->width = width;
            ++state->height;
            ++state->progress;
        }
    }
}

// ---- a wide level: four launches ----
__device__ __forceinline__ bool wide_level(const RcmState* st) {
    return st->open && !st->pending && !st->error && st->width > kNarrow;
}

template <int LANES>
__global__ __launch_bounds__(kBlock)
void rcm_wide_parents_kernel(const int* __restrict__ rp, const int* __restrict__ ci, const int* __restrict__ queue,
                             const int* mark, unsigned long long* pkey, const RcmState* __restrict__ state) {
    if (!wide_level(state)) return;
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int start = state->start, width = state->width, epoch = state->epoch;
    for (long long r = static_cast<long long>(blockIdx.x) * kRows + threadIdx.x / LANES; r < width;
         r += static_cast<long long>(gridDim.x) * kRows) {
        const int u = queue[start + r];
        offer_row<LANES>(rp[u], rp[u + 1], lane, epoch, start + static_cast<int>(r), ci, mark, pkey);
    }
}

// count[r] = the children of the level's rows before r inside r's chunk of kRows rows; chunk_sum[c] = chunk c's children
template <int LANES>
__global__ __launch_bounds__(kBlock)
void rcm_wide_counts_kernel(const int* __restrict__ rp, const int* __restrict__ ci, const int* __restrict__ queue,
                            const unsigned long long* pkey, int* __restrict__ count, int* __restrict__ chunk_sum,
                            const RcmState* __restrict__ state) {
    if (!wide_level(state)) return;
    constexpr int kRows = kBlock / LANES;
    __shared__ int s_cnt[kBlock];
    __shared__ int s_off[kBlock];
    __shared__ int s_wave[kBlock / 64];
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    const int start = state->start, width = state->width, epoch = state->epoch;
    const long long chunks = (static_cast<long long>(width) + kRows - 1) / kRows;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long r = c * kRows + slot;
        const bool active = r < width;
        const int u = active ? queue[start + r] : 0;
        const int mine = walk_children<LANES>(active, active ? rp[u] : 0, active ? rp[u + 1] : 0, lane, epoch,
                                              start + static_cast<int>(r), ci, pkey, [](int, int) {});
        s_cnt[threadIdx.x] = 0;
        __syncthreads();
        if (active && lane == 0) s_cnt[slot] = mine;
        __syncthreads();
        const int total = block_exclusive_scan(s_cnt, s_off, s_wave);
        if (active && lane == 0) count[r] = s_off[slot];
        if (threadIdx.x == 0) chunk_sum[c] = total;
        __syncthreads();
    }
}

// One workgroup: the exclusive scan of the chunk totals in place, then the next level's place in the queue, or the
// end of the sweep when the level has no children.
__global__ __launch_bounds__(kBlock)
void rcm_wide_scan_kernel(int n, int rows_per_chunk, const int* __restrict__ queue, int* __restrict__ chunk_sum,
                          RcmState* state, int peripheral) {
    if (!wide_level(state)) return;
    __shared__ int s_cnt[kBlock];
    __shared__ int s_off[kBlock];
    __shared__ int s_wave[kBlock / 64];
    const int start = state->start, width = state->width;
    const int chunks = (width + rows_per_chunk - 1) / rows_per_chunk;
    const int next = start + width;
    long long running = 0;
    for (int first = 0; first < chunks; first += kBlock) {
        const int c = first + static_cast<int>(threadIdx.x);
        s_cnt[threadIdx.x] = c < chunks ? chunk_sum[c] : 0;
        __syncthreads();
        const int total = block_exclusive_scan(s_cnt, s_off, s_wave);
        if (c < chunks) chunk_sum[c] = static_cast<int>(min(running, static_cast<long long>(n))) + s_off[threadIdx.x];
        running += total;
    }
    if (running > n - next) {
        if (threadIdx.x == 0) state->error = 1;
        return;
    }
    if (running == 0) {
        int m = INT_MAX;
        for (int i = threadIdx.x; i < width; i += kBlock) m = min(m, queue[start + i]);
        m = block_min_all(m, s_wave);
        if (threadIdx.x == 0) close_sweep(state, peripheral, m);
        return;
    }
    if (threadIdx.x == 0) {
        state->next_start = next;
        state->next_width = static_cast<int>(running);
        state->pending = 1;
        ++state->height;
        ++state->progress;
    }
}

template <int LANES>
__global__ __launch_bounds__(kBlock)
void rcm_wide_children_kernel(int n, const int* __restrict__ rp, const int* __restrict__ ci, int* queue, int* mark,
                              const unsigned long long* pkey, const int* __restrict__ count,
                              const int* __restrict__ chunk_sum, const RcmState* __restrict__ state) {
    if (!state->pending || state->error) return;                  // the scan of this round found children
    constexpr int kRows = kBlock / LANES;
    const int lane = threadIdx.x % LANES;
    const int slot = threadIdx.x / LANES;
    const int start = state->start, width = state->width, epoch = state->epoch;
    const int stamp = state->final_sweep ? kNumbered : epoch;
    const int next = state->next_start;
    const long long chunks = (static_cast<long long>(width) + kRows - 1) / kRows;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long r = c * kRows + slot;
        const bool active = r < width;
        const int u = active ? queue[start + r] : 0;
        const int slice = active ? next + chunk_sum[c] + count[r] : 0;
        walk_children<LANES>(active, active ? rp[u] : 0, active ? rp[u + 1] : 0, lane, epoch,
                             start + static_cast<int>(r), ci, pkey, [&](int rank, int x) {
                                 const int at = slice + rank;
                                 if (at >= 0 && at < n) {
                                     queue[at] = x;
                                     mark[x] = stamp;
                                 }
                             });
    }
}

// the Cuthill-McKee sequence taken back through D and reversed
__global__ __launch_bounds__(kBlock) void rcm_output_kernel(int n, const int* __restrict__ queue,
                                                            const int* __restrict__ by_key, int* __restrict__ perm,
                                                            int* __restrict__ inverse) {
    for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kBlock) {
        const int old = by_key[queue[i]];
        const int at = n - 1 - static_cast<int>(i);
        perm[at] = old;
        inverse[old] = at;
    }
}

// ---- band statistics ----
struct BandPartial {
    int lower, upper;
    long long profile;
};

template <int LANES>
__global__ __launch_bounds__(kBlock)
void band_kernel(int rows, const int* __restrict__ rp, const int* __restrict__ ci, BandPartial* __restrict__ partial) {
    constexpr int kRows = kBlock / LANES;
    __shared__ int s_lower[kBlock / 64], s_upper[kBlock / 64];
    __shared__ long long s_profile[kBlock / 64];
    const int lane = threadIdx.x % LANES;
    int lower = 0, upper = 0;
    long long profile = 0;
    for (long long first = static_cast<long long>(blockIdx.x) * kRows; first < rows;
         first += static_cast<long long>(gridDim.x) * kRows) {
        const long long row = first + threadIdx.x / LANES;
        int lowest = INT_MAX;
        if (row < rows) {
            const int i = static_cast<int>(row);
            const int end = rp[i + 1];
            for (int j = rp[i] + lane; j < end; j += LANES) {
                const int c = ci[j];
                lower = max(lower, i - c);
                upper = max(upper, c - i);
                lowest = min(lowest, c);
            }
        }
#pragma unroll
        for (int off = LANES / 2; off > 0; off >>= 1) lowest = min(lowest, __shfl_xor(lowest, off, 64));
        if (row < rows && lane == 0 && lowest < row) profile += row - lowest;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lower = max(lower, __shfl_xor(lower, off, 64));
        upper = max(upper, __shfl_xor(upper, off, 64));
        profile += __shfl_xor(profile, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_lower[threadIdx.x >> 6] = lower;
        s_upper[threadIdx.x >> 6] = upper;
        s_profile[threadIdx.x >> 6] = profile;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            lower = max(lower, s_lower[w]);
            upper = max(upper, s_upper[w]);
            profile += s_profile[w];
        }
        partial[blockIdx.x] = BandPartial{lower, upper, profile};
    }
}

// one workgroup: out = the fold of partial[0, count)
__global__ __launch_bounds__(kBlock) void band_fold_kernel(const BandPartial* __restrict__ partial, int count,
                                                           BandPartial* __restrict__ out) {
    __shared__ int s_lower[kBlock / 64], s_upper[kBlock / 64];
    __shared__ long long s_profile[kBlock / 64];
    int lower = 0, upper = 0;
    long long profile = 0;
    for (int i = threadIdx.x; i < count; i += kBlock) {
        lower = max(lower, partial[i].lower);
        upper = max(upper, partial[i].upper);
        profile += partial[i].profile;
    }
    for (int off = 32; off > 0; off >>= 1) {
        lower = max(lower, __shfl_xor(lower, off, 64));
        upper = max(upper, __shfl_xor(upper, off, 64));
        profile += __shfl_xor(profile, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_lower[threadIdx.x >> 6] = lower;
        s_upper[threadIdx.x >> 6] = upper;
        s_profile[threadIdx.x >> 6] = profile;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) {
            lower = max(lower, s_lower[w]);
            upper = max(upper, s_upper[w]);
            profile += s_profile[w];
        }
        *out = BandPartial{lower, upper, profile};
    }
}

// a CSRMatrix of the library's own, destroyed with the scope
struct OwnedCsr {
    CSRMatrix* m = csr_create(0, 0, 0);
    ~OwnedCsr() { csr_destroy(m); }
    OwnedCsr() = default;
    OwnedCsr(const OwnedCsr&) = delete;
    OwnedCsr& operator=(const OwnedCsr&) = delete;
};

int flag_read(const int* d_flag, hipStream_t s, int* value) {
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(value, d_flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    return 0;
}

// the ordering on `s`; the checks of rcm_check have passed and A has rows
int order(const CSRMatrix* A, int* d_perm, int* d_inverse, const RcmConfig& cfg, RcmResult* result, hipStream_t s) {
    const int n = A->num_rows;
    // ---- the device checks, before anything walks the structure ----
    int status = structure_checked(A, s);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    DevBuf<int> flag;
    if (dev_alloc(&flag, 1) != hipSuccess) return fail(result, SpMVError::CUDA_MALLOC);
    int unsorted = 0;
    if (hipMemsetAsync(flag.get(), 0, sizeof(int), s) != hipSuccess) return fail(result, SpMVError::KERNEL_LAUNCH);
    rcm_ascending_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, A->d_row_ptrs, A->d_col_indices, flag.get());
    status = flag_read(flag.get(), s, &unsorted);
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    if (unsorted) return fail(result, SpMVError::INVALID_FORMAT);

    // ---- S, the vertices by key, S' ----
    OwnedCsr transposed, summed, renumbered;
    if (!transposed.m || !summed.m || !renumbered.m) return fail(result, SpMVError::CUDA_MALLOC);
    const CSRMatrix* S = A;
    if (!cfg.symmetric_pattern) {
        status = csr_transpose_gpu(transposed.m, A);
        if (status == 0) status = csr_add(summed.m, 1.0f, A, 1.0f, transposed.m);
        if (status != 0) return fail(result, static_cast<SpMVError>(status));
        csr_free_gpu(transposed.m);
        S = summed.m;
    }
    DevBuf<int> degree, by_key, key_of;
    if (dev_alloc(&degree, n) != hipSuccess || dev_alloc(&by_key, n) != hipSuccess ||
        dev_alloc(&key_of, n) != hipSuccess) {
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    rcm_degree_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, S->d_row_ptrs, S->d_col_indices, degree.get());
    if (hipGetLastError() != hipSuccess) return fail(result, SpMVError::KERNEL_LAUNCH);
    // the stable counting sort by degree (a degree is below n)
    status = color_ordering(n, degree.get(), n, by_key.get(), key_of.get(), nullptr);
    if (status == 0) status = csr_permute_gpu(renumbered.m, S, by_key.get(), key_of.get());
    if (status != 0) return fail(result, static_cast<SpMVError>(status));
    csr_free_gpu(summed.m);
    key_of.reset();
    const CSRMatrix* G = renumbered.m;

    // ---- the loop ----
    solver::Workspace<RcmState> ws;
    DevBuf<int> queue, mark, count, chunk_sum;
    DevBuf<unsigned long long> pkey;
    const size_t ints = static_cast<size_t>(n) * sizeof(int);
    if (!ws.allocate(0, 0) || dev_alloc(&queue, n) != hipSuccess || dev_alloc(&mark, n) != hipSuccess ||
        dev_alloc(&count, n) != hipSuccess || dev_alloc(&chunk_sum, static_cast<long long>(n) + 1) != hipSuccess ||
        dev_alloc(&pkey, n) != hipSuccess) {
        return fail(result, SpMVError::CUDA_MALLOC);
    }
    const TraceRange range("spmv:csr_rcm");
    const int lanes = cfg.lanes_per_row != 0
                          ? cfg.lanes_per_row
                          : pick_lanes_per_row(static_cast<float>(G->nnz) / static_cast<float>(n));
    const int rows_per_chunk = kBlock / lanes;
    const int grid = capped_grid(n, rows_per_chunk);
    EventPair& ev = thread_events();
    if (!ev.start || !ev.stop || hipEventRecord(ev.start, s) != hipSuccess) return fail(result, SpMVError::KERNEL_LAUNCH);
    bool ok = hipMemsetAsync(ws.state, 0, sizeof(RcmState), s) == hipSuccess &&
              hipMemsetAsync(mark.get(), 0, ints, s) == hipSuccess &&
              hipMemsetAsync(pkey.get(), 0xff, static_cast<size_t>(n) * sizeof(unsigned long long), s) == hipSuccess;
    if (ok) {
        rcm_init_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, degree.get(), by_key.get(), queue.get(), mark.get(), ws.state);
        ok = hipGetLastError() == hipSuccess;
        ++result->launches;
    }
    const int* rp = G->d_row_ptrs;
    const int* ci = G->d_col_indices;
    bool finished = false;
    int progress = -1;
    while (ok && !finished) {
        for (int t = 0; t < kRoundsPerBatch && ok; ++t) {
            ok = with_lanes(lanes, [&](auto L) {
                constexpr int kLanes = decltype(L)::value;
                rcm_run_kernel<kLanes><<<1, kBlock, 0, s>>>(n, rp, ci, queue.get(), mark.get(), pkey.get(), ws.state,
                                                            cfg.peripheral);
                rcm_wide_parents_kernel<kLanes><<<grid, kBlock, 0, s>>>(rp, ci, queue.get(), mark.get(), pkey.get(),
                                                                        ws.state);
                rcm_wide_counts_kernel<kLanes><<<grid, kBlock, 0, s>>>(rp, ci, queue.get(), pkey.get(), count.get(),
                                                                       chunk_sum.get(), ws.state);
                rcm_wide_scan_kernel<<<1, kBlock, 0, s>>>(n, rows_per_chunk, queue.get(), chunk_sum.get(), ws.state,
                                                          cfg.peripheral);
                rcm_wide_children_kernel<kLanes><<<grid, kBlock, 0, s>>>(n, rp, ci, queue.get(), mark.get(),
                                                                         pkey.get(), count.get(), chunk_sum.get(),
                                                                         ws.state);
                return hipGetLastError();
            }) == hipSuccess;
            result->launches += 5;
        }
        ok = ws.read_back(ok, s);
        if (!ok) break;
        const RcmState& st = ws.pinned[0];
        // a batch that numbered no level and closed no sweep: a broken invariant ends the call, it never hangs
        if (st.error || (!st.finished && st.progress == progress)) ok = false;
        progress = st.progress;
        finished = st.finished != 0;
    }
    if (ok) {
        rcm_output_kernel<<<vec_grid(n), kBlock, 0, s>>>(n, queue.get(), by_key.get(), d_perm, d_inverse);
        ok = hipGetLastError() == hipSuccess;
        ++result->launches;
    }
    if (!ws.finish_timed(ok, ev, s, &result->elapsed_ms)) {
        (void)hipStreamSynchronize(s);                            // the scratch is freed after the last kernel
        return fail(result, SpMVError::KERNEL_LAUNCH);
    }
    result->components = ws.pinned[0].components;
    result->levels = ws.pinned[0].levels;
    result->sweeps = ws.pinned[0].sweeps;
    return 0;
}

int band(const CSRMatrix* A, CsrBand* out, hipStream_t s) {
    const int rows = A->num_rows;
    if (rows == 0 || A->nnz == 0) {
        if (rows > 0) {
            const int status = structure_checked(A, s);
            if (status != 0) return status;
        }
        *out = CsrBand{0, 0, 0};
        return 0;
    }
    const int status = structure_checked(A, s);
    if (status != 0) return status;
    const int lanes = pick_lanes_per_row(static_cast<float>(A->nnz) / static_cast<float>(rows));
    const int grid = capped_grid(rows, kBlock / lanes);
    DevBuf<BandPartial> partial;
    if (dev_alloc(&partial, static_cast<long long>(grid) + 1) != hipSuccess) return fail(SpMVError::CUDA_MALLOC);
    const hipError_t launched = with_lanes(lanes, [&](auto L) {
        band_kernel<decltype(L)::value><<<grid, kBlock, 0, s>>>(rows, A->d_row_ptrs, A->d_col_indices, partial.get());
        return hipGetLastError();
    });
    band_fold_kernel<<<1, kBlock, 0, s>>>(partial.get(), grid, partial.get() + grid);
    BandPartial total{0, 0, 0};
    if (launched != hipSuccess || hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&total, partial.get() + grid, sizeof(total), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        return fail(SpMVError::KERNEL_LAUNCH);
    }
    *out = CsrBand{total.lower, total.upper, total.profile};
    return 0;
}

} // namespace

} // namespace rcm
} // namespace detail

RcmResult csr_rcm(const CSRMatrix* A, int* d_perm, int* d_inverse, const RcmConfig* config) {
    using namespace detail;
    RcmResult result;
    const RcmConfig defaults;
    const RcmConfig& cfg = config ? *config : defaults;
    bool nothing = false;
    result.error_code = rcm::rcm_check(A, d_perm, d_inverse, cfg, &nothing);
    if (result.error_code != 0 || nothing) return result;
    rcm::order(A, d_perm, d_inverse, cfg, &result, current_stream());
    return result;
}

RcmResult rcm_reorder(CSRMatrix* B, const CSRMatrix* A, int* d_perm, int* d_inverse, const RcmConfig* config) {
    using namespace detail;
    RcmResult result;
    if (!B || !A || !d_perm || !d_inverse || B == A) {
        result.error_code = code(SpMVError::INVALID_ARGUMENT);
        return result;
    }
    result = csr_rcm(A, d_perm, d_inverse, config);
    if (result.error_code != 0) return result;
    result.error_code = csr_permute_gpu(B, A, d_perm, d_inverse);
    return result;
}

int csr_band_gpu(const CSRMatrix* A, CsrBand* out) {
    using namespace detail;
    const int status = rcm::band_check(A, out);
    if (status != 0) return status;
    return rcm::band(A, out, current_stream());
}

} // namespace spmv
