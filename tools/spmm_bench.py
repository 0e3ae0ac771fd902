"""spmm_bench.py — spmv_csr_multi (Y = A * X, k right-hand sides) against k calls of the best single-vector route.

Matrices are built in HBM by the device generators: C2 (uniform 1 M x 1 M, 16 entries per row) and C4 (power-law row
lengths, 1 M rows).  X is filled by spmv_c_gen_vector.  Every figure is the median of --runs device-event times
(the elapsed_ms each call reports) after --warmup calls.  The single-vector baseline is the fastest of direct
spmv_csr with every kernel type and of the LDS-tiled engine (use_texture), promotion off; `ratio` is one multi call
over k of those calls.  Prints one JSON object (and writes it to --out when given).

    python tools/spmm_bench.py [--runs 20] [--warmup 5] [--out FILE]
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

KS = (1, 2, 4, 8, 16, 32, 64)
KERNELS = {"SCALAR_CSR": 0, "VECTOR_CSR": 1, "MERGE_PATH": 2}


def median_ms(call, warmup, runs):
    for _ in range(warmup):
        call()
    return statistics.median(call() for _ in range(runs))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    n = args.rows

    def checked(res):
        if res.error_code != 0:
            raise RuntimeError(spmv.spmv_error_string(res.error_code))
        return float(res.elapsed_ms)

    result = {"tool": "tools/spmm_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "statistic": "median device-event ms per call", "matrices": {}}
    for name, make in (("C2", lambda: wl.uniform_csr_device(42, n, n, 16)),
                       ("C4", lambda: wl.power_law_csr_device(42, n, n))):
        A = make()
        x, y = wl.vector_device(42, 1, A.cols), spmv.CudaBuffer(A.rows)
        single = {}
        for kname, kt in KERNELS.items():
            cfg = spmv.SpMVConfig(kt)
            single["direct " + kname] = median_ms(lambda: checked(spmv.spmv_csr(A.handle, x, y, cfg, A.cols)),
                                                  args.warmup, args.runs)
        for kname in ("VECTOR_CSR", "MERGE_PATH"):
            cfg = spmv.SpMVConfig(KERNELS[kname], 256, True)
            single["use_texture " + kname] = median_ms(lambda: checked(spmv.spmv_csr(A.handle, x, y, cfg, A.cols)),
                                                       args.warmup, args.runs)
        best_route = min(single, key=single.get)
        best = single[best_route]
        x.release()
        y.release()
        spmv.csr_invalidate_gpu_cache(A.handle)          # drop the tiled plan before the multi runs
        entry = {"rows": A.rows, "cols": A.cols, "nnz": A.nnz,
                 "single_vector_ms": {k: round(v, 5) for k, v in single.items()},
                 "best_single_route": best_route, "best_single_ms": round(best, 5), "multi": {}}
        for k in KS:
            X = wl.vector_device(42, 100 + k, A.cols * k)
            Y = spmv.CudaBuffer(A.rows * k)
            row = {"k_x_best_single_ms": round(k * best, 5)}
            for kname, kt in KERNELS.items():
                cfg = spmv.SpMVConfig(kt)
                ms = median_ms(lambda: checked(spmv.spmv_csr_multi(A.handle, X, Y, k, config=cfg, vec_size=A.cols)),
                               args.warmup, args.runs)
                bw = spmv.compute_bandwidth_csr_multi(A.handle, k, ms).achieved_bandwidth_gb_s
                row[kname] = {"ms": round(ms, 5), "ratio": round(ms / (k * best), 4), "gb_s": round(bw, 1)}
            entry["multi"][str(k)] = row
            X.release()
            Y.release()
        result["matrices"][name] = entry
        A.close()

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
