// ppr_smoke.cpp — a C++ caller of pagerank_personalized written the way the reference's tests are: `#include
// "spmv/*.h"`, namespace spmv, CudaBuffer.  A ring of 64 nodes with chords (every column sums to 1) and one dangling
// node; k = 3 teleport vectors in a layout with padding (ldv = 3, ldr = 5): every column of the result is a
// distribution, a column equals the k = 1 call on it bit for bit, the seeds entry point equals the explicit V, the
// padding of R stays as it was.  Then the argument errors.  Built with plain g++ against include/ and libspmv_amd.so
// by tests/test_gpu_ppr.py.  Needs a GPU.
#include "spmv/cuda_buffer.h"
#include "spmv/pagerank.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// node c links to c + 1 and c + 5 (mod n), each with weight 1/2; node 9 links to nobody
static CSRMatrix* ring(int n) {
    std::vector<std::vector<int>> in(n);
    for (int c = 0; c < n; ++c) {
        if (c == 9) continue;
        in[(c + 1) % n].push_back(c);
        in[(c + 5) % n].push_back(c);
    }
    CSRMatrix* A = csr_create(n, n, 2 * (n - 1));
    int at = 0;
    for (int r = 0; r < n; ++r) {
        A->row_ptrs[r] = at;
        for (int c : in[r]) {
            A->col_indices[at] = c;
            A->values[at++] = 0.5f;
        }
    }
    A->row_ptrs[n] = at;
    return A;
}

int main() {
    const int n = 64, k = 3, ldv = 3, ldr = 5;
    CSRMatrix* A = ring(n);
    CHECK(csr_to_gpu(A) == 0);
    const float pad = -123.5f;
    std::vector<float> V(static_cast<size_t>(n) * ldv, 0.0f), R(static_cast<size_t>(n) * ldr, pad);
    V[7 * ldv + 0] = 1.0f;                                   // one node
    V[9 * ldv + 1] = 1.0f;                                   // the dangling node
    for (int i = 0; i < n; ++i) V[i * ldv + 2] = 1.0f / n;   // everyone
    CudaBuffer<float> d_V(V.size()), d_R(R.size()), d_v(n), d_r(n);
    d_V.copyFromHost(V.data(), V.size());
    d_R.copyFromHost(R.data(), R.size());

    PageRankConfig cfg;
    cfg.tolerance = 1e-6f;
    PersonalizedResult results[3];
    CHECK(pagerank_personalized(A, d_V.get(), ldv, d_R.get(), ldr, k, &cfg, results) == 0);
    d_R.copyToHost(R.data(), R.size());
    for (int j = 0; j < k; ++j) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += R[i * ldr + j];
        CHECK(results[j].error_code == 0 && results[j].converged == 1 && std::fabs(sum - 1.0) < 1e-5);
        CHECK(results[j].elapsed_ms == results[0].elapsed_ms);
        std::vector<float> v(n), r(n);
        for (int i = 0; i < n; ++i) v[i] = V[i * ldv + j];
        d_v.copyFromHost(v.data(), n);
        PersonalizedResult one;
        CHECK(pagerank_personalized(A, d_v.get(), 1, d_r.get(), 1, 1, &cfg, &one) == 0);
        d_r.copyToHost(r.data(), n);
        int differ = 0;
        for (int i = 0; i < n; ++i) differ += std::memcmp(&R[i * ldr + j], &r[i], sizeof(float)) != 0;
        CHECK(differ == 0 && one.iterations == results[j].iterations && one.converged == results[j].converged);
        CHECK(std::memcmp(&one.final_residual, &results[j].final_residual, sizeof(float)) == 0);
        std::printf("column %d: %d iterations, residual %.3g, sum %.9f, %d rows differ from the k = 1 call\n", j,
                    results[j].iterations, results[j].final_residual, sum, differ);
    }
    CHECK(results[1].iterations == 1 && results[0].iterations > 1);
    CHECK(R[9 * ldr + 1] == 1.0f);
    int pad_written = 0;
    for (int i = 0; i < n; ++i) {
        for (int j = k; j < ldr; ++j) pad_written += R[i * ldr + j] != pad;
    }
    CHECK(pad_written == 0);

    // the seeds entry point: {7}, {9}, everyone
    std::vector<int> ptrs = {0, 1, 2, 2 + n}, nodes = {7, 9};
    for (int i = 0; i < n; ++i) nodes.push_back(i);
    std::vector<float> R2(R.size(), pad);
    CudaBuffer<float> d_R2(R2.size());
    d_R2.copyFromHost(R2.data(), R2.size());
    PersonalizedResult seeded[3];
    CHECK(pagerank_personalized_seeds(A, ptrs.data(), nodes.data(), k, d_R2.get(), ldr, &cfg, seeded) == 0);
    d_R2.copyToHost(R2.data(), R2.size());
    CHECK(std::memcmp(R.data(), R2.data(), R.size() * sizeof(float)) == 0);
    for (int j = 0; j < k; ++j) CHECK(seeded[j].iterations == results[j].iterations);

    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(pagerank_personalized(nullptr, d_V.get(), ldv, d_R.get(), ldr, k, nullptr, results) == invalid_argument);
    results[0].error_code = 77;
    CHECK(pagerank_personalized(A, d_V.get(), ldv, d_R.get(), ldr, 33, nullptr, results) == invalid_argument);
    CHECK(results[0].error_code == 77);      // k out of range: `results` is not touched
    CHECK(pagerank_personalized(A, d_V.get(), 2, d_R.get(), ldr, k, nullptr, results) == invalid_argument);
    CHECK(pagerank_personalized(A, d_V.get(), ldv, d_V.get(), ldv, k, nullptr, results) == invalid_argument);
    PageRankConfig bad;
    bad.damping_factor = 1.0f;
    CHECK(pagerank_personalized(A, d_V.get(), ldv, d_R.get(), ldr, k, &bad, results) == invalid_argument);
    CHECK(results[2].error_code == invalid_argument);
    nodes[1] = n;                             // out of range
    CHECK(pagerank_personalized_seeds(A, ptrs.data(), nodes.data(), k, d_R2.get(), ldr, &cfg, seeded) == invalid_argument);
    V[3 * ldv + 0] = -0.5f;                   // a negative entry: refused on the device, R untouched
    d_V.copyFromHost(V.data(), V.size());
    CHECK(pagerank_personalized(A, d_V.get(), ldv, d_R2.get(), ldr, k, &cfg, results) == invalid_argument);
    std::vector<float> R3(R2.size());
    d_R2.copyToHost(R3.data(), R3.size());
    CHECK(std::memcmp(R2.data(), R3.data(), R2.size() * sizeof(float)) == 0);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
