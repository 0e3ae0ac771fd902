// spmv/pagerank.h — PageRank power iteration on top of the CSR SpMV.
//
// Same API as the reference (include/spmv/pagerank.h:9-43).  The loop itself
// is device-resident here: one fused kernel per iteration (SpMV + damping +
// teleport + residual and dangling-mass partial sums), no PCIe copies inside
// the loop.  Row-sharded multi-GPU operation goes through the shard API below.
#ifndef SPMV_PAGERANK_H
#define SPMV_PAGERANK_H

#include "csr_matrix.h"

#include <vector>

namespace spmv {

struct PageRankConfig {
    float damping_factor;
    float tolerance;
    int   max_iterations;

    PageRankConfig() : damping_factor(0.85f), tolerance(1e-6f), max_iterations(100) {}
};

struct PageRankResult {
    float* ranks;            // new float[num_nodes]; release with pagerank_free
    int    iterations;
    float  final_residual;   // L2 norm of the last update
    bool   converged;

    PageRankResult() : ranks(nullptr), iterations(0), final_residual(0.0f), converged(false) {}
};

// adj_matrix: column-normalised adjacency in CSR (row i = in-links of node i).
// Extension: with SPMV_NUM_GPUS=N (N > 1) in the environment and host arrays present, the call runs
// pagerank_multi_gpu(adj_matrix, config, N) instead; unset, behaviour is the reference's single-device one.
PageRankResult pagerank(const CSRMatrix* adj_matrix, const PageRankConfig* config = nullptr);

// Extension (the reference is single-GPU): the same iteration with the CSR rows sharded
// over `num_gpus` devices of this process — contiguous row blocks cut for equal nnz (binary search on
// row_ptrs), every device a full-length rank vector, ONE RCCL all-gather of the new slices per iteration
// (single-process ncclCommInitAll, one stream per device).  Shards are cut from the HOST arrays; the matrix
// need not be resident on any device.  Same result contract as pagerank(): ranks released by pagerank_free;
// an empty result (ranks == nullptr) when fewer than num_gpus devices or no RCCL are available.
PageRankResult pagerank_multi_gpu(const CSRMatrix* adj_matrix, const PageRankConfig* config, int num_gpus);
// the row boundaries it cuts (num_shards + 1 ascending row indices, bounds[0] = 0, bounds[num_shards] = num_rows)
std::vector<int> pagerank_shard_bounds(const int* row_ptrs, int num_rows, int num_shards);

void pagerank_free(PageRankResult* result);

struct TopKNode {
    int   node_id;
    float rank;
};

void pagerank_top_k(const PageRankResult* result, int num_nodes, int k, TopKNode* top_k);

// ---- personalized PageRank, k teleport vectors in one matrix pass per step (extension) ----
// Per column j, with d = damping_factor and `dangling` the mask pagerank() computes:
//     r_0      = v_j
//     s        = float(sum of r_old over the dangling nodes)               (fp64 partials, fixed-order fold)
//     r_new[i] = (d * (A r_old)[i] + (d * s) * v_j[i]) + (1 - d) * v_j[i]  (every operation rounded on its own)
//     stop when ||r_new - r_old||_2 < tolerance (as pagerank()) or after max_iterations
//     result   = last committed vector divided by its sum
// The loop is device-resident and runs on the direct kernels only (it never touches the matrix's tiled plan).  Column
// j is bit for bit the k = 1 call on V[:, j], whatever the other columns hold and whatever ldv, ldr and the
// alignment are; with n a power of two and V[:, j] = 1/n it is bit for bit pagerank() on the direct kernels.  A
// converged column is frozen while the others run; the call ends when every column is done or max_iterations steps
// are enqueued.  Same bits on every run.  Runs on spmv_get_stream() and returns after completion; call it outside a
// graph capture.
struct PersonalizedResult {
    int   error_code;      // SpMVError as int
    int   iterations;      // committed steps of this column
    float final_residual;  // ||r_new - r_old||_2 of this column's last committed step
    int   converged;
    float elapsed_ms;      // device-event time of the batched loop, the same in every entry
};

// d_V: num_rows x k teleport distributions, row-major, leading dimension ldv >= k, on the device (read only).
// d_R: num_rows x k ranks out, row-major, ldr >= k, on the device: written once, at the end; columns k..ldr-1 are
// never written.  1 <= k <= 32.  results: k entries.
// Checks, in this order, before any device work (a failing one writes nothing to d_R and only error_code in results;
// a k out of range writes nothing in results either):
//   1. adj, d_V, d_R or results null -> INVALID_ARGUMENT     5. num_rows == 0 -> SUCCESS, every column converged, 0 iterations
//   2. k < 1 or k > 32 -> INVALID_ARGUMENT                   6. device arrays missing -> INVALID_FORMAT
//   3. ldv < k or ldr < k -> INVALID_ARGUMENT                7. damping outside (0, 1), tolerance < 0 or not finite,
//   4. not square -> INVALID_DIMENSION                          max_iterations < 0 -> INVALID_ARGUMENT (null config: defaults)
//   8. the ranges of d_V and d_R overlap -> INVALID_ARGUMENT
// and one on the device, in the setup pass: a column of V with a negative or non-finite entry, or whose sum is not
// > 0, fails the whole call with INVALID_ARGUMENT, d_R untouched.
int pagerank_personalized(const CSRMatrix* adj, const float* d_V, int ldv, float* d_R, int ldr, int k,
                          const PageRankConfig* config, PersonalizedResult* results);

// Convenience: column j teleports uniformly to seed_nodes[seed_ptrs[j] .. seed_ptrs[j+1]) (host arrays).  Builds V
// on the device (a fill kernel, value 1.0f / count) and calls the above.  An empty set, a node out of range or a
// node listed twice in one set -> INVALID_ARGUMENT, checked on the host before any device work.
int pagerank_personalized_seeds(const CSRMatrix* adj, const int* seed_ptrs, const int* seed_nodes, int k,
                                float* d_R, int ldr, const PageRankConfig* config, PersonalizedResult* results);

} // namespace spmv

#endif // SPMV_PAGERANK_H
