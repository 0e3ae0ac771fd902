"""cg_bench.py — cg_solve time per iteration against spmv_csr, per engine, on the two benchmark matrices.

Matrices (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu):
* P3D: the 7-point 3-D Poisson matrix at 160^3 (4.1 M rows, 28 M entries; banded, local gathers);
* RSPD: the random SPD matrix S + S^T + D at 4 M rows and 15 entries per row (scattered gathers).
Plus P2D64 (5-point 2-D Poisson at 64^2), where the launch latency dominates.

Per matrix and engine (0 direct, 1 tiled where eligible): --runs solves of exactly --iters iterations (tolerance 0,
JACOBI) after one warm-up solve; ms per iteration = median elapsed_ms / iters.  Beside it the median spmv_csr time
with the same engine (VECTOR_CSR; use_texture for engine 1; promotion off), the byte model of one iteration and the
issue's target 1.3 x (spmv + 48 B/row / 5.0 TB/s).  A converging solve (tolerance 1e-6, engine -1) is reported too.
--merge-stats NAME=CSV[,NAME=CSV] adds each matrix's per-kernel split from a `rocprofv3 --kernel-trace --stats` run
of this tool on that matrix alone (kernels shared by the matrices would mix otherwise).

    python tools/cg_bench.py [--matrices P3D,RSPD,P2D64] [--iters 100] [--runs 3] [--out FILE]
                             [--merge-stats P3D=a.csv,RSPD=b.csv]
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TARGET_BPS = 5.0e12


def kernel_split(path):
    """{kernel: {calls, avg_us, total_ms}} from a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            short = name.split("(anonymous namespace)::", 1)[-1].split("(")[0].split("::")[-1]
            short = short[5:] if short.startswith("void ") else short
            out[short] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 3),
                          "total_ms": round(float(row["TotalDurationNs"]) / 1e6, 3)}
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="P3D,RSPD,P2D64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spmv-runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    makers = {"P3D": lambda: spd.poisson3d(160), "RSPD": lambda: spd.random_spd(4_000_000, 7, seed=42),
              "P2D64": lambda: spd.poisson2d(64)}
    result = {"tool": "tools/cg_bench.py", "device": spmv.device_name(), "iters": args.iters, "runs": args.runs,
              "statistic": "median over runs; ms_per_iter = elapsed_ms / iters (tolerance 0, JACOBI)",
              "launches_per_iter": {"direct": 3, "tiled": "2 (tiled_spmv) + 3"}, "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        b = spmv.CudaBuffer(n)
        b.copyFromHost(np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32), n)
        x, y = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        zeros = np.zeros(n, np.float32)
        spmv_bytes = nnz * 8 + (n + 1) * 4 + 2 * n * 4           # entries, row pointers, x gathered once, y
        entry = {"rows": n, "nnz": nnz, "tiled_eligible": bool(spmv.tiled_shape(n, n, nnz)[0]),
                 "bytes_model": {"spmv": spmv_bytes,
                                 "cg_direct": spmv_bytes + 44 * n,  # update 28 B/row, direction 16 B/row
                                 "cg_tiled": spmv_bytes + 52 * n},  # + the p.q kernel's 8 B/row
                 "engines": {}}
        for engine in (0, 1):
            if engine == 1 and not entry["tiled_eligible"]:
                continue
            cfg = spmv.CGConfig(tolerance=0.0, max_iterations=args.iters, preconditioner=1, engine=engine)
            times = []
            for run in range(args.runs + 1):
                x.copyFromHost(zeros, n)
                res = spmv.cg_solve(A, b, x, cfg)
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run:
                    times.append(res.elapsed_ms / max(res.iterations, 1))
            ms_iter = statistics.median(times)
            t_spmv = statistics.median(wl.time_spmv_csr(A, b, y, 1, warmup=5, runs=args.spmv_runs,
                                                        use_texture=engine == 1))
            target = 1.3 * (t_spmv + 48.0 * n / HBM_TARGET_BPS * 1e3)
            model = entry["bytes_model"]["cg_tiled" if engine == 1 else "cg_direct"]
            entry["engines"][str(engine)] = {
                "ms_per_iter": round(ms_iter, 5), "spmv_csr_ms": round(t_spmv, 5),
                "target_ms": round(target, 5), "meets_target": ms_iter <= target,
                "iter_over_spmv": round(ms_iter / t_spmv, 3),
                "model_tb_s": round(model / (ms_iter * 1e-3) / 1e12, 3)}
        x.copyFromHost(zeros, n)
        spmv.csr_invalidate_gpu_cache(A)
        res = spmv.cg_solve(A, b, x, spmv.CGConfig(tolerance=1e-6, max_iterations=5000))
        entry["converge_auto_1e-6"] = {"iterations": res.iterations, "converged": res.converged,
                                       "relative_residual": res.relative_residual,
                                       "elapsed_ms": round(res.elapsed_ms, 3),
                                       "plan_cached_after": spmv.csr_has_tiled_plan(A)}
        for buf in (b, x, y):
            buf.release()
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    for pair in filter(None, (args.merge_stats or "").split(",")):
        name, path = pair.split("=", 1)
        if name in result["matrices"]:
            result["matrices"][name]["kernel_stats"] = kernel_split(path)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
