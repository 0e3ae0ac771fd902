// rcm_host.cpp — the host side of the reverse Cuthill-McKee calls of include/spmv/reorder.h that needs no device
// (DESIGN.md §4.28): csr_rcm_cpu, the definition of the ordering, written as the plain sequential queue algorithm;
// csr_band_cpu; and the argument checks of the device entry points in rcm.hip.
#include "rcm_impl.h"
#include "internal.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace spmv {
namespace detail {
namespace rcm {

namespace {

bool lanes_ok(int lanes) { return lanes == 0 || (lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0); }

bool config_ok(const RcmConfig& cfg) {
    return lanes_ok(cfg.lanes_per_row) && (cfg.peripheral == 0 || cfg.peripheral == 1) && cfg.reserved == 0;
}

// csr_transpose_gpu's structure rule on host arrays; `ascending`: and every column strictly above its left neighbour
bool structure_ok(const CSRMatrix* A, bool ascending) {
    const int rows = A->num_rows;
    if (A->row_ptrs[0] != 0 || A->row_ptrs[rows] != A->nnz) return false;
    for (int i = 0; i < rows; ++i) {
        if (A->row_ptrs[i + 1] < A->row_ptrs[i]) return false;
    }
    for (int j = 0; j < A->nnz; ++j) {
        if (A->col_indices[j] < 0 || A->col_indices[j] >= A->num_cols) return false;
    }
    if (ascending) {
        for (int i = 0; i < rows; ++i) {
            for (int j = A->row_ptrs[i] + 1; j < A->row_ptrs[i + 1]; ++j) {
                if (A->col_indices[j] <= A->col_indices[j - 1]) return false;
            }
        }
    }
    return true;
}

// The graph of the definition: row v of (ptr, adj) is adj(v) in ascending key.
struct Graph {
    int n = 0;
    std::vector<int> ptr, adj, deg;
    std::vector<int> stamp;             // stamp[v] == epoch: v is in the level structure being built
    std::vector<char> numbered;
    int epoch = 0;

    bool before(int a, int b) const { return deg[a] < deg[b] || (deg[a] == deg[b] && a < b); }

    // the rooted level structure L(r) over the unnumbered vertices: its level count, and the vertex of smallest key in
    // its last level
    void level_structure(int r, int* levels, int* last_min) {
        ++epoch;
        std::vector<int> level{r}, next;
        stamp[r] = epoch;
        int count = 0;
        while (true) {
            ++count;
            next.clear();
            for (int u : level) {
                for (int j = ptr[u]; j < ptr[u + 1]; ++j) {
                    const int w = adj[j];
                    if (numbered[w] || stamp[w] == epoch) continue;
                    stamp[w] = epoch;
                    next.push_back(w);
                }
            }
            if (next.empty()) break;
            level.swap(next);
        }
        int best = level[0];
        for (int v : level) {
            if (before(v, best)) best = v;
        }
        *levels = count;
        *last_min = best;
    }
};

void build_graph(const CSRMatrix* A, int symmetric_pattern, Graph* g) {
    const int n = A->num_rows;
    const int* rp = A->row_ptrs;
    const int* ci = A->col_indices;
    std::vector<uint64_t> edges;                                   // (v, u): u in adj(v)
    edges.reserve(static_cast<size_t>(A->nnz) * (symmetric_pattern ? 1 : 2));
    for (int v = 0; v < n; ++v) {
        for (int j = rp[v]; j < rp[v + 1]; ++j) {
            const int u = ci[j];
            if (u == v) continue;
            edges.push_back((static_cast<uint64_t>(v) << 32) | static_cast<unsigned>(u));
            if (!symmetric_pattern) edges.push_back((static_cast<uint64_t>(u) << 32) | static_cast<unsigned>(v));
        }
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    g->n = n;
    g->ptr.assign(static_cast<size_t>(n) + 1, 0);
    g->adj.resize(edges.size());
    for (uint64_t e : edges) ++g->ptr[static_cast<size_t>(e >> 32) + 1];
    for (int v = 0; v < n; ++v) g->ptr[v + 1] += g->ptr[v];
    for (size_t k = 0; k < edges.size(); ++k) g->adj[k] = static_cast<int>(edges[k] & 0xffffffffu);
    g->deg.resize(static_cast<size_t>(n));
    for (int v = 0; v < n; ++v) g->deg[v] = g->ptr[v + 1] - g->ptr[v];
    for (int v = 0; v < n; ++v) {
        std::sort(g->adj.begin() + g->ptr[v], g->adj.begin() + g->ptr[v + 1],
                  [g](int a, int b) { return g->before(a, b); });
    }
    g->stamp.assign(static_cast<size_t>(n), 0);
    g->numbered.assign(static_cast<size_t>(n), 0);
}

} // namespace

int rcm_check(const CSRMatrix* A, const int* d_perm, const int* d_inverse, const RcmConfig& cfg, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_perm || !d_inverse) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return 0;
    }
    // (csr_color's rule: a negative nnz fails)
    if (A->num_rows < 0 || A->nnz < 0 || !A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    if (!lanes_ok(cfg.lanes_per_row)) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.peripheral != 0 && cfg.peripheral != 1) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.reserved != 0) return code(SpMVError::INVALID_ARGUMENT);
    return 0;
}

int band_check(const CSRMatrix* A, const CsrBand* out) {
    if (!A || !out) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

} // namespace rcm
} // namespace detail

int csr_rcm_cpu(const CSRMatrix* A, int* perm, int* inverse, int* components, int* levels, const RcmConfig* config) {
    using namespace detail;
    using namespace detail::rcm;
    if (!A || !perm || !inverse) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) {
        if (components) *components = 0;
        if (levels) *levels = 0;
        return code(SpMVError::SUCCESS);
    }
    if (n < 0 || A->nnz < 0 || !A->row_ptrs || (A->nnz > 0 && !A->col_indices)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const RcmConfig defaults;
    const RcmConfig& cfg = config ? *config : defaults;
    if (!config_ok(cfg)) return code(SpMVError::INVALID_ARGUMENT);
    if (!structure_ok(A, true)) return code(SpMVError::INVALID_FORMAT);

    Graph g;
    build_graph(A, cfg.symmetric_pattern, &g);
    std::vector<int> by_key(static_cast<size_t>(n));
    for (int v = 0; v < n; ++v) by_key[v] = v;
    std::sort(by_key.begin(), by_key.end(), [&g](int a, int b) { return g.before(a, b); });

    std::vector<int> order;                                        // the Cuthill-McKee sequence, which is also the queue
    order.reserve(static_cast<size_t>(n));
    int count = 0, total_levels = 0;
    size_t cursor = 0;
    while (order.size() < static_cast<size_t>(n)) {
        while (g.numbered[by_key[cursor]]) ++cursor;
        int r = by_key[cursor];
        int height = 0, c = r;
        g.level_structure(r, &height, &c);
        while (cfg.peripheral) {
            int height_c = 0, next_c = c;
            g.level_structure(c, &height_c, &next_c);
            if (height_c <= height) break;
            r = c;
            height = height_c;
            c = next_c;
        }
        size_t head = order.size();
        order.push_back(r);
        g.numbered[r] = 1;
        while (head < order.size()) {
            const int u = order[head++];
            for (int j = g.ptr[u]; j < g.ptr[u + 1]; ++j) {        // ascending key
                const int w = g.adj[j];
                if (g.numbered[w]) continue;
                g.numbered[w] = 1;
                order.push_back(w);
            }
        }
        ++count;
        total_levels += height;
    }
    for (int i = 0; i < n; ++i) {
        const int old = order[static_cast<size_t>(n) - 1 - i];
        perm[i] = old;
        inverse[old] = i;
    }
    if (components) *components = count;
    if (levels) *levels = total_levels;
    return code(SpMVError::SUCCESS);
}

int csr_band_cpu(const CSRMatrix* A, CsrBand* out) {
    using namespace detail;
    if (!A || !out) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows < 0 || A->num_cols < 0 || A->nnz < 0) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows == 0) {
        if (A->nnz != 0) return code(SpMVError::INVALID_FORMAT);
        *out = CsrBand{0, 0, 0};
        return code(SpMVError::SUCCESS);
    }
    if (!A->row_ptrs || (A->nnz > 0 && !A->col_indices)) return code(SpMVError::INVALID_ARGUMENT);
    if (!rcm::structure_ok(A, false)) return code(SpMVError::INVALID_FORMAT);
    CsrBand band{0, 0, 0};
    for (int i = 0; i < A->num_rows; ++i) {
        int first = i;
        for (int j = A->row_ptrs[i]; j < A->row_ptrs[i + 1]; ++j) {
            const int c = A->col_indices[j];
            band.lower = std::max(band.lower, i - c);
            band.upper = std::max(band.upper, c - i);
            first = std::min(first, c);
        }
        band.profile += i - first;
    }
    *out = band;
    return code(SpMVError::SUCCESS);
}

} // namespace spmv
