"""ic0_bench.py — ic0_csr factorisation time, and cg_solve_ic against cg_solve JACOBI to the same answer.

Matrices (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu):
* P3D: the 7-point Laplacian poisson3d(160) (4.1 M rows; 478 levels, wide in the middle);
* P2D64: the 5-point Laplacian poisson2d(64) (127 levels of at most 64 rows: single-workgroup launches).

Per matrix:
* factorisation: the LOWER schedule is prebuilt by sptrsv_analyze (its analysis_ms is reported), then --runs
  ic0_csr calls after one warm-up; the figure is the median elapsed_ms (device events around the factorisation's
  launches).  Beside it levels, launches, lanes, the time of ic0_cpu_csr on this host, and the launch term
  launches x t_launch, t_launch being the per-launch time of a one-element fill kernel enqueued --launch-probe times
  back to back in this run (what sptrsv_bench.py takes);
* solves at --tolerance (1e-6) from x0 = 0, engine 0, median of --runs after one warm-up each: cg_solve_ic with that
  factor and cg_solve JACOBI, the same b: iterations, elapsed_ms / iterations (ms per step), elapsed_ms
  (ms to solution; the factorisation time is listed separately and is not included), the true relative residual in
  fp64, the launches of one preconditioned step's two triangular solves and their launch term.

    python tools/ic0_bench.py [--matrices P3D,P2D64] [--runs 3] [--out FILE]
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
    ap.add_argument("--launch-probe", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    # per-launch time of a (nearly) empty kernel, back to back on the default stream
    probe = spmv.CudaBuffer(1)
    for _ in range(100):
        spmv.lib().spmv_c_fill(probe.get(), 1, 0.0, None)
    spmv.device_synchronize()
    t0 = time.perf_counter()
    for _ in range(args.launch_probe):
        spmv.lib().spmv_c_fill(probe.get(), 1, 0.0, None)
    spmv.device_synchronize()
    launch_ms = (time.perf_counter() - t0) * 1e3 / args.launch_probe
    probe.release()

    makers = {"P3D": lambda: spd.poisson3d(160), "P2D64": lambda: spd.poisson2d(64)}
    result = {"tool": "tools/ic0_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "tolerance": args.tolerance,
              "statistic": "median over runs after one warm-up; schedules prebuilt; engine 0; x0 = 0",
              "launch_ms": round(launch_ms, 5), "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        factor = spmv.CudaBuffer(nnz)
        ahead = [spmv.sptrsv_analyze(A, uplo) for uplo in (0, 1)]
        for a in ahead:
            if a.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(a.error_code))
        t0 = time.perf_counter()
        spmv.ic0_cpu_csr(A)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        times = []
        for run in range(args.runs + 1):
            res = spmv.ic0_csr(A, factor)
            if res.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(res.error_code))
            if run:
                times.append(float(res.elapsed_ms))
        entry = {"rows": n, "nnz": nnz,
                 "ic0": {"ms": round(statistics.median(times), 5), "analysis_ms": round(float(ahead[0].analysis_ms), 3),
                          "num_levels": res.num_levels, "launches": res.launches, "lanes_per_row": res.lanes_per_row,
                          "bad_pivot": res.bad_pivot, "cpu_ms": round(cpu_ms, 3),
                          "launch_term_ms": round(res.launches * launch_ms, 5)}}
        F = spmv.csr_wrap_device(n, n, nnz, A.contents.d_row_ptrs, A.contents.d_col_indices, factor.get())
        b_host = np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32)
        b, x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(b_host, n)
        zeros = np.zeros(n, np.float32)
        b64 = b_host.astype(np.float64)
        solve_launches = ahead[0].launches + ahead[1].launches            # z: LOWER, then UPPER
        for label, run_solver in (
                ("ic0", lambda cfg: spmv.cg_solve_ic(A, F, b, x, cfg)),
                ("jacobi", lambda cfg: spmv.cg_solve(A, b, x, cfg))):
            cfg = spmv.CGConfig(tolerance=args.tolerance, max_iterations=5000, preconditioner=1, engine=0)
            elapsed = []
            for run in range(args.runs + 1):
                x.copyFromHost(zeros, n)
                res = run_solver(cfg)
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run:
                    elapsed.append(float(res.elapsed_ms))
            ms = statistics.median(elapsed)
            r = b64 - spd.spmv64(rp, ci, va, x.copyToHost(n))
            entry["cg_" + label] = {
                "iterations": res.iterations, "converged": int(res.converged), "breakdown": res.breakdown,
                "ms_to_solution": round(ms, 5), "ms_per_step": round(ms / max(res.iterations, 1), 5),
                "true_relative_residual": float(np.linalg.norm(r) / np.linalg.norm(b64))}
        entry["cg_ic0"]["solve_launches_per_step"] = solve_launches
        entry["cg_ic0"]["solve_launch_term_ms_per_step"] = round(solve_launches * launch_ms, 5)
        entry["ic0_over_jacobi_ms_to_solution"] = round(
            entry["cg_ic0"]["ms_to_solution"] / entry["cg_jacobi"]["ms_to_solution"], 3)
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
