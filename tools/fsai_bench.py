"""fsai_bench.py — fsai_csr / fsai_csr_numeric times, and cg_solve_fsai against cg_solve JACOBI and cg_solve_ic to the
same answer.

Matrices (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu):
* P3D: the 7-point Laplacian poisson3d(160) (4.1 M rows);
* P2D64: the 5-point Laplacian poisson2d(64).

Per matrix and per pattern (S = A, and S = A*A from spgemm_csr):
* setup: --runs fsai_csr calls and --runs fsai_csr_numeric calls after one warm-up each; the figures are the median
  elapsed_ms (device events around the structure build + numeric kernel, and around the numeric kernel + bad-row scan).
  Beside them G's entries, the longest row, the row class and the lanes; the time of csr_transpose_gpu(GT, G) on the
  host clock; for S = A*A the spgemm_csr time;
* solves at --tolerance (1e-6) from x0 = 0, engine 0, median of --runs after one warm-up each, the same b in the same
  process: cg_solve_fsai with that G and GT, cg_solve JACOBI, cg_solve_ic with ic0_csr's factor (schedules prebuilt):
  iterations, elapsed_ms / iterations (ms per step), elapsed_ms (ms to solution; setup times are listed separately and
  are not included) and the true relative residual in fp64.

    python tools/fsai_bench.py [--matrices P3D,P2D64] [--runs 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="P3D,P2D64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    def check(code):
        if code != 0:
            raise RuntimeError(spmv.spmv_error_string(code))

    makers = {"P3D": lambda: spd.poisson3d(160), "P2D64": lambda: spd.poisson2d(64)}
    result = {"tool": "tools/fsai_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "tolerance": args.tolerance,
              "statistic": "median over runs after one warm-up; engine 0; x0 = 0; setup not in ms_to_solution",
              "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        check(spmv.csr_to_gpu(A))
        b_host = np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32)
        b, x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(b_host, n)
        zeros = np.zeros(n, np.float32)
        b64 = b_host.astype(np.float64)
        entry = {"rows": n, "nnz": nnz}

        def solve(label, run_solver):
            cfg = spmv.CGConfig(tolerance=args.tolerance, max_iterations=5000, preconditioner=1, engine=0)
            elapsed = []
            for run in range(args.runs + 1):
                x.copyFromHost(zeros, n)
                res = run_solver(cfg)
                check(res.error_code)
                if run:
                    elapsed.append(float(res.elapsed_ms))
            ms = statistics.median(elapsed)
            r = b64 - spd.spmv64(rp, ci, va, x.copyToHost(n))
            entry[label] = {
                "iterations": res.iterations, "converged": int(res.converged), "breakdown": res.breakdown,
                "ms_to_solution": round(ms, 5), "ms_per_step": round(ms / max(res.iterations, 1), 5),
                "true_relative_residual": float(np.linalg.norm(r) / np.linalg.norm(b64))}

        for pattern in ("A", "AA"):
            S = None
            setup = {}
            if pattern == "AA":
                S = spmv.csr_create(1, 1, 0)
                product = spmv.spgemm_csr(S, A, A)
                check(product.error_code)
                setup["spgemm_ms"] = round(float(product.symbolic_ms + product.numeric_ms), 5)
            G, GT = spmv.csr_create(1, 1, 0), spmv.csr_create(1, 1, 0)
            built, refilled = [], []
            for run in range(args.runs + 1):
                res = spmv.fsai_csr(G, A, S)
                check(res.error_code)
                if run:
                    built.append(float(res.elapsed_ms))
            for run in range(args.runs + 1):
                again = spmv.fsai_csr_numeric(G, A)
                check(again.error_code)
                if run:
                    refilled.append(float(again.elapsed_ms))
            spmv.device_synchronize()
            t0 = time.perf_counter()
            check(spmv.csr_transpose_gpu(GT, G))
            spmv.device_synchronize()
            setup.update({"fsai_csr_ms": round(statistics.median(built), 5),
                          "fsai_csr_numeric_ms": round(statistics.median(refilled), 5),
                          "transpose_ms": round((time.perf_counter() - t0) * 1e3, 3),
                          "g_nnz": res.nnz, "max_row": res.max_row, "row_class": res.row_class,
                          "lanes_per_row": res.lanes_per_row, "bad_row": res.bad_row})
            entry["fsai_" + pattern] = setup
            solve("cg_fsai_" + pattern, lambda cfg: spmv.cg_solve_fsai(A, G, GT, b, x, cfg))
            for M in (S, G, GT):
                spmv.csr_destroy(M)

        solve("cg_jacobi", lambda cfg: spmv.cg_solve(A, b, x, cfg))
        factor = spmv.CudaBuffer(nnz)
        for uplo in (0, 1):
            check(spmv.sptrsv_analyze(A, uplo).error_code)
        check(spmv.ic0_csr(A, factor).error_code)
        F = spmv.csr_wrap_device(n, n, nnz, A.contents.d_row_ptrs, A.contents.d_col_indices, factor.get())
        solve("cg_ic0", lambda cfg: spmv.cg_solve_ic(A, F, b, x, cfg))
        for other in ("cg_jacobi", "cg_ic0"):
            for pattern in ("A", "AA"):
                entry[f"fsai_{pattern}_over_{other[3:]}_ms_to_solution"] = round(
                    entry["cg_fsai_" + pattern]["ms_to_solution"] / entry[other]["ms_to_solution"], 3)
        for buf in (b, x, factor):
            buf.release()
        spmv.csr_destroy(F)
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
