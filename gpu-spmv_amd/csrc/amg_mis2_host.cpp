// amg_mis2_host.cpp — amg_aggregate_mis2_cpu_csr, the sequential definition of the MIS-2 aggregation that
// amg_setup_device runs on the device (include/spmv/amg.h).  Host only: no device call.
#include "amg_impl.h"
#include "internal.h"
#include "reorder_impl.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace spmv {

namespace {

using detail::amg_strong;
using detail::code;
using detail::reorder::higher_priority;

enum : char { UNDECIDED = 0, ROOT = 1, OUT = 2 };

struct Graph {
    int n;
    const int* rp;
    const int* ci;
    const float* va;
    std::vector<float> d;
    double theta2;

    bool strong(int i, int p) const { return amg_strong(i, ci[p], va[p], theta2, d[i], d[ci[p]]); }

    // calls visit(u) for every u of N2(v), possibly more than once, until it returns false
    template <class Visit>
    void two_hop(int v, Visit&& visit) const {
        for (int p = rp[v]; p < rp[v + 1]; ++p) {
            if (!strong(v, p)) continue;
            const int u = ci[p];
            if (!visit(u)) return;
            for (int q = rp[u]; q < rp[u + 1]; ++q) {
                if (strong(u, q) && ci[q] != v && !visit(ci[q])) return;
            }
        }
    }
};

// the roots: the vertices in descending priority, each a root iff no root is in its N2 yet
void select_roots(const Graph& g, unsigned seed, std::vector<char>* state) {
    std::vector<int> order(static_cast<size_t>(g.n));
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [seed](int a, int b) { return higher_priority(a, b, seed); });
    state->assign(static_cast<size_t>(g.n), UNDECIDED);
    for (const int v : order) {
        bool root = true;
        g.two_hop(v, [&](int u) {
            if ((*state)[u] == ROOT) root = false;
            return root;
        });
        (*state)[v] = root ? ROOT : OUT;
    }
}

// the rounds of the loop that reads the states of the round before
int synchronous_rounds(const Graph& g, unsigned seed) {
    std::vector<char> state(static_cast<size_t>(g.n), UNDECIDED);
    std::vector<int> waiting(static_cast<size_t>(g.n));
    std::iota(waiting.begin(), waiting.end(), 0);
    std::vector<std::pair<int, char>> decided;
    int rounds = 0;
    while (!waiting.empty()) {
        ++rounds;
        decided.clear();
        std::vector<int> still;
        for (const int v : waiting) {
            bool saw_root = false, saw_undecided = false;
            g.two_hop(v, [&](int u) {
                if (higher_priority(u, v, seed)) {
                    if (state[u] == ROOT) saw_root = true;
                    else if (state[u] == UNDECIDED) saw_undecided = true;
                }
                return !saw_root;
            });
            if (saw_root) decided.emplace_back(v, OUT);
            else if (!saw_undecided) decided.emplace_back(v, ROOT);
            else still.push_back(v);
        }
        for (const auto& change : decided) state[change.first] = change.second;
        waiting.swap(still);
    }
    return rounds;
}

} // namespace

int amg_aggregate_mis2_cpu_csr(const CSRMatrix* A, float strength, unsigned seed, int* aggregate_out,
                               int* num_aggregates, int* rounds) {
    if (!A || !aggregate_out || !num_aggregates) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n < 0 || A->nnz < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values)) ||
        !detail::amg_structure_ok(n, A->nnz, A->row_ptrs, A->col_indices)) {
        return code(SpMVError::INVALID_FORMAT);
    }
    if (!(strength >= 0.0f)) return code(SpMVError::INVALID_ARGUMENT);

    Graph g{n, A->row_ptrs, A->col_indices, A->values, {}, static_cast<double>(strength) * static_cast<double>(strength)};
    detail::amg_diagonal(n, g.rp, g.ci, g.va, &g.d, nullptr);
    std::vector<char> state;
    select_roots(g, seed, &state);

    // numbers: the roots by ascending row; phase 1: the first root of N(i) in storage order
    std::vector<int> first(static_cast<size_t>(n), -1);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        if (state[i] == ROOT) first[i] = count++;
    }
    for (int i = 0; i < n; ++i) {
        if (state[i] == ROOT) continue;
        for (int p = g.rp[i]; p < g.rp[i + 1]; ++p) {
            if (g.strong(i, p) && state[g.ci[p]] == ROOT) {
                first[i] = first[g.ci[p]];
                break;
            }
        }
    }
    // phase 2: membership as of the end of phase 1
    for (int i = 0; i < n; ++i) {
        int best = -1;
        float best_abs = 0.0f;
        if (first[i] == -1) {
            for (int p = g.rp[i]; p < g.rp[i + 1]; ++p) {
                if (!g.strong(i, p) || first[g.ci[p]] == -1) continue;
                const float a = std::fabs(g.va[p]);
                if (best == -1 || a > best_abs) {
                    best = g.ci[p];
                    best_abs = a;
                }
            }
        }
        aggregate_out[i] = best != -1 ? first[best] : first[i];
    }
    *num_aggregates = count;
    if (rounds) *rounds = synchronous_rounds(g, seed);
    return 0;
}

} // namespace spmv
