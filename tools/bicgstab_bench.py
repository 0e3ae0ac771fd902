"""bicgstab_bench.py — bicgstab_solve time per iteration against spmv_csr, per engine, on the two benchmark matrices.

Matrices (numpy, gpu-spmv_amd/nonsym.py, uploaded with csr_from_arrays + csr_to_gpu):
* CD3D: 3-D convection-diffusion at 160^3, wind 1 on every axis (4.1 M rows, 28.5 M entries; the structure of
  cg_bench.py's P3D, so the two solvers compare directly);
* RNS: the random non-symmetric matrix at 4 M rows and 15 off-diagonal entries per row (scattered gathers).
Plus CD2D64 (2-D convection-diffusion at 64^2), where the launch latency dominates: reported only.

Per matrix and engine (0 direct, 1 tiled where eligible): --runs solves of exactly --iters iterations (tolerance 0,
JACOBI) after one warm-up solve; ms per iteration = median elapsed_ms / iters.  Beside it the median spmv_csr time
with the same engine (VECTOR_CSR; use_texture for engine 1; promotion off), the byte model of one iteration and the
target 1.3 x (2 spmv + element-wise bytes / 5.0 TB/s).  Element-wise bytes per row with JACOBI, from the kernels:
  direct  84 = r^ read by the first fused SpMV 4 + s kernel 20 (v, r, dinv in; s, s^ out) + s read by the second
          fused SpMV 4 + update 32 (p^, s^, t, r^, x, s in; x, r out) + direction 24 (v, r, dinv, p in; p, p^ out)
  tiled   92 = the same with the two dot kernels reading both of their vectors (8 + 8 instead of 4 + 4)
A converging solve (tolerance 1e-6, engine -1) is reported too.  --merge-stats NAME=CSV[,NAME=CSV] adds each
matrix's per-kernel split from a `rocprofv3 --kernel-trace --stats` run of this tool on that matrix alone.

    python tools/bicgstab_bench.py [--matrices CD3D,RNS,CD2D64] [--iters 100] [--runs 3] [--out FILE]
                                   [--merge-stats CD3D=a.csv,RNS=b.csv]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cg_bench import HBM_TARGET_BPS, kernel_split  # noqa: E402

ELEMENTWISE_BYTES_PER_ROW = {"direct": 84, "tiled": 92}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="CD3D,RNS,CD2D64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spmv-runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    makers = {"CD3D": lambda: nonsym.convdiff3d(160, 1.0), "RNS": lambda: nonsym.random_nonsym(4_000_000, 15, seed=42),
              "CD2D64": lambda: nonsym.convdiff2d(64, 1.0)}
    result = {"tool": "tools/bicgstab_bench.py", "device": spmv.device_name(), "iters": args.iters,
              "runs": args.runs,
              "statistic": "median over runs; ms_per_iter = elapsed_ms / iters (tolerance 0, JACOBI)",
              "launches_per_iter": {"direct": 5, "tiled": "2 x (2 (tiled_spmv) + 1 dot) + 3"},
              "elementwise_bytes_per_row": ELEMENTWISE_BYTES_PER_ROW, "matrices": {}}
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
                                 "bicgstab_direct": 2 * spmv_bytes + ELEMENTWISE_BYTES_PER_ROW["direct"] * n,
                                 "bicgstab_tiled": 2 * spmv_bytes + ELEMENTWISE_BYTES_PER_ROW["tiled"] * n},
                 "engines": {}}
        for engine in (0, 1):
            if engine == 1 and not entry["tiled_eligible"]:
                continue
            kind = "tiled" if engine == 1 else "direct"
            cfg = spmv.BiCGStabConfig(tolerance=0.0, max_iterations=args.iters, preconditioner=1, engine=engine)
            times, res = [], None
            for run in range(args.runs + 1):
                x.copyFromHost(zeros, n)
                res = spmv.bicgstab_solve(A, b, x, cfg)
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run:
                    times.append(res.elapsed_ms / max(res.iterations, 1))
            ms_iter = statistics.median(times)
            t_spmv = statistics.median(wl.time_spmv_csr(A, b, y, 1, warmup=5, runs=args.spmv_runs,
                                                        use_texture=engine == 1))
            target = 1.3 * (2 * t_spmv + ELEMENTWISE_BYTES_PER_ROW[kind] * n / HBM_TARGET_BPS * 1e3)
            model = entry["bytes_model"]["bicgstab_" + kind]
            entry["engines"][str(engine)] = {
                "ms_per_iter": round(ms_iter, 5), "iterations_run": res.iterations, "breakdown": res.breakdown,
                "spmv_csr_ms": round(t_spmv, 5), "target_ms": round(target, 5), "meets_target": ms_iter <= target,
                "iter_over_2spmv": round(ms_iter / (2 * t_spmv), 3),
                "model_tb_s": round(model / (ms_iter * 1e-3) / 1e12, 3)}
        x.copyFromHost(zeros, n)
        spmv.csr_invalidate_gpu_cache(A)
        res = spmv.bicgstab_solve(A, b, x, spmv.BiCGStabConfig(tolerance=1e-6, max_iterations=5000))
        entry["converge_auto_1e-6"] = {"iterations": res.iterations, "converged": res.converged,
                                       "breakdown": res.breakdown, "relative_residual": res.relative_residual,
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
