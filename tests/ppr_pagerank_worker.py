"""Child process of tests/test_gpu_ppr.py: started with SPMV_TILED=0 (read once per process), so that pagerank() stays
on the direct kernels.  A non-dyadic graph of n nodes (n a power of two; synth.uniform_csr, column-stochastic, three
dangling nodes), damping 0.85, tolerance 1e-6; pagerank_personalized with k = 3, column 1 = 1 / n between two seeded
columns.  Column 1 must equal pagerank() bit for bit: ranks, iterations, final_residual, converged."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("SPMV_TILED") == "0"
    n = int(sys.argv[1])
    assert n & (n - 1) == 0
    gpu = importlib.import_module("gpu-spmv_amd")
    gpu.require_gpu()
    dangling = (5, 1000, n - 7)
    rp, ci, _ = gpu.synth.uniform_csr(n, 0, n, n, 9)
    keep = ~np.isin(ci, np.array(dangling, np.int32))
    counts = np.add.reduceat(keep.astype(np.int64), rp[:-1])
    ci = ci[keep]
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    va = gpu.synth.column_stochastic_values(ci, n)
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    cfg = gpu.PageRankConfig(0.85, 1e-6, 100)
    ref = gpu.pagerank(A, cfg)
    assert not gpu.csr_has_tiled_plan(A)

    V = np.zeros((n, 3), np.float32)
    V[17, 0] = 1.0
    V[:, 1] = np.float32(1.0) / np.float32(n)
    V[[5, 900], 2] = 0.5
    d_V, d_R = gpu.CudaBuffer(3 * n), gpu.CudaBuffer(3 * n)
    d_V.copyFromHost(V.ravel(), 3 * n)
    results = gpu.pagerank_personalized(A, d_V, d_R, 3, config=cfg)
    R = d_R.copyToHost(3 * n).reshape(n, 3)
    r = results[1]
    print("pagerank():", ref.iterations, ref.final_residual, ref.converged, " column 1:", r.iterations, r.final_residual,
          r.converged, " other columns:", [(x.iterations, x.converged) for x in (results[0], results[2])])
    assert all(x.error_code == 0 for x in results)
    assert (r.iterations, bool(r.converged)) == (ref.iterations, bool(ref.converged)) and ref.converged
    assert np.float32(r.final_residual).view(np.uint32) == np.float32(ref.final_residual).view(np.uint32)
    differ = np.flatnonzero(np.ascontiguousarray(R[:, 1]).view(np.uint32) != ref.ranks.view(np.uint32))
    assert differ.size == 0, (differ[:8], R[differ[:8], 1], ref.ranks[differ[:8]])
    ref1 = gpu.pagerank(A, gpu.PageRankConfig(0.85, 0.0, 1))          # one step: the host-summed starting dangling mass
    one = gpu.pagerank_personalized(A, d_V, d_R, 3, config=gpu.PageRankConfig(0.85, 0.0, 1))
    R = d_R.copyToHost(3 * n).reshape(n, 3)
    assert one[1].iterations == ref1.iterations == 1
    assert np.float32(one[1].final_residual).view(np.uint32) == np.float32(ref1.final_residual).view(np.uint32)
    assert np.array_equal(np.ascontiguousarray(R[:, 1]).view(np.uint32), ref1.ranks.view(np.uint32))
    gpu.csr_destroy(A)
    print("column 1 equals pagerank()")


if __name__ == "__main__":
    main()
