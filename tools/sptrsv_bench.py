"""sptrsv_bench.py — sptrsv_csr time per solve against a launch + bandwidth model, on three matrices.

Matrices (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu):
* P3D: the 7-point 3-D Poisson matrix at 160^3 (4.1 M rows; 478 levels by the 3m - 2 rule, wide in the middle);
* RSPD: the random SPD matrix S + S^T + D at 4 M rows and 7 + 7 + 1 entries per row (cg_bench.py's);
* P2D64: the 5-point 2-D Poisson matrix at 64^2 (127 levels of at most 64 rows: one single-workgroup launch).

Per matrix, LOWER and UPPER, NON_UNIT, ordered 0 and 1: the schedule is prebuilt by sptrsv_analyze (its analysis_ms is
reported), then --runs solves after one warm-up; the figure is the median elapsed_ms (device events around the solve's
launches).  Beside it: num_levels and launches; the time of sptrsv_cpu_csr on this host; and a model
    launches x t_launch + triangle_bytes / rate
where t_launch is the per-launch time of a one-element fill kernel (the library's nearest thing to an empty kernel)
enqueued --launch-probe times back to back in this run, rate is what spmv_csr VECTOR_CSR reaches on the same matrix
in this run by its own byte model, and triangle_bytes = 8 per stored entry of the full rows walked + 4 (n + 1) row
pointers + 4 n order + 12 n vectors (b, x written, x gathered).  ratio = measured / model.

    python tools/sptrsv_bench.py [--matrices P3D,RSPD,P2D64] [--runs 3] [--out FILE]
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
    ap.add_argument("--matrices", default="P3D,RSPD,P2D64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--spmv-runs", type=int, default=20)
    ap.add_argument("--launch-probe", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
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

    makers = {"P3D": lambda: spd.poisson3d(160), "RSPD": lambda: spd.random_spd(4_000_000, 7, seed=42),
              "P2D64": lambda: spd.poisson2d(64)}
    result = {"tool": "tools/sptrsv_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "statistic": "median elapsed_ms over runs after one warm-up, schedule prebuilt by sptrsv_analyze",
              "launch_ms": round(launch_ms, 5), "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        b_host = np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32)
        b, x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(b_host, n)
        t_spmv = statistics.median(wl.time_spmv_csr(A, b, x, 1, warmup=5, runs=args.spmv_runs))
        spmv_bytes = nnz * 8 + (n + 1) * 4 + 2 * n * 4
        rate = spmv_bytes / (t_spmv * 1e-3)
        tri_bytes = 8 * nnz + 4 * (n + 1) + 4 * n + 12 * n
        entry = {"rows": n, "nnz": nnz, "spmv_csr_vector_ms": round(t_spmv, 5),
                 "spmv_rate_tb_s": round(rate / 1e12, 3), "triangle_bytes": tri_bytes, "solves": {}}
        for uplo in (0, 1):
            ahead = spmv.sptrsv_analyze(A, uplo)
            if ahead.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(ahead.error_code))
            t0 = time.perf_counter()
            spmv.sptrsv_cpu_csr(A, b_host, spmv.SpTRSVConfig(uplo=uplo))
            cpu_ms = (time.perf_counter() - t0) * 1e3
            for ordered in (0, 1):
                cfg = spmv.SpTRSVConfig(uplo=uplo, diag=0, ordered=ordered)
                times = []
                for run in range(args.runs + 1):
                    res = spmv.sptrsv_csr(A, b, x, cfg)
                    if res.error_code != 0:
                        raise RuntimeError(spmv.spmv_error_string(res.error_code))
                    if run:
                        times.append(float(res.elapsed_ms))
                ms = statistics.median(times)
                model_launch = res.launches * launch_ms
                model_bytes = tri_bytes / rate * 1e3
                entry["solves"][f"{'upper' if uplo else 'lower'}_ordered{ordered}"] = {
                    "ms": round(ms, 5), "analysis_ms": round(float(ahead.analysis_ms), 3),
                    "num_levels": res.num_levels, "launches": res.launches, "lanes_per_row": res.lanes_per_row,
                    "cpu_ms": round(cpu_ms, 3), "model_launch_ms": round(model_launch, 5),
                    "model_bytes_ms": round(model_bytes, 5), "model_ms": round(model_launch + model_bytes, 5),
                    "ratio_to_model": round(ms / (model_launch + model_bytes), 3)}
        for buf in (b, x):
            buf.release()
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
