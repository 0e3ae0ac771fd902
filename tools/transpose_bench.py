"""transpose_bench.py — csr_transpose_gpu build time and steady-state spmv_csr_transpose against spmv_csr.

Matrices are built in HBM by the device generators: C2 (uniform 1 M x 1 M, 16 entries per row), C4 (power-law row
lengths, 1 M rows, max 10 000) and C5 (uniform 10 M x 10 M, 160 M entries).  x is filled by spmv_c_gen_vector.

* build: csr_transpose_gpu into a fresh matrix, --builds times; `span_ms` is the device-event time from before the
  call to after it on the library stream (kernels plus the host's flag read and allocations in between), `wall_ms`
  the call's host time.  Kernel-only time comes from a `rocprofv3 --kernel-trace --stats` run of this tool:
  --merge-stats FILE adds the transpose kernels' totals from its kernel_stats.csv, per build.
* steady state: the median of --runs elapsed_ms after --warmup calls, per kernel type, of spmv_csr_transpose(A),
  spmv_csr on the explicit transpose (same config) and spmv_csr(A); promotion off.

    python tools/transpose_bench.py [--runs 20] [--warmup 5] [--builds 5] [--out FILE] [--merge-stats CSV]
"""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"SCALAR_CSR": (0, False), "VECTOR_CSR": (1, False), "MERGE_PATH": (2, False),
           "MERGE_PATH use_texture": (2, True)}


def median_ms(call, warmup, runs):
    for _ in range(warmup):
        call()
    return statistics.median(call() for _ in range(runs))


def kernel_totals(path, builds_per_matrix):
    """{kernel: {calls, total_ms}} of the transpose kernels in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "transpose_" not in name:
                continue
            short = name.split("transpose_")[1].split("(")[0]
            out["transpose_" + short] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return {"per_kernel": out, "builds": builds_per_matrix}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--matrices", default="C2,C4,C5")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()

    import torch

    spmv = importlib.import_module("gpu-spmv_amd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    def checked(res):
        if res.error_code != 0:
            raise RuntimeError(spmv.spmv_error_string(res.error_code))
        return float(res.elapsed_ms)

    makers = {"C2": lambda: wl.uniform_csr_device(42, 1_000_000, 1_000_000, 16),
              "C4": lambda: wl.power_law_csr_device(42, 1_000_000, 1_000_000),
              "C5": lambda: wl.uniform_csr_device(42, 10_000_000, 10_000_000, 16)}
    result = {"tool": "tools/transpose_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "builds": args.builds,
              "statistic": "median; build: device-event span and host wall time per call; spmv: elapsed_ms",
              "matrices": {}}
    for name in args.matrices.split(","):
        A = makers[name]()
        entry = {"rows": A.rows, "cols": A.cols, "nnz": A.nnz}
        spans, walls = [], []
        for _ in range(args.builds + 1):                   # the first build warms the allocator and the code objects
            AT = spmv.csr_create(0, 0, 0)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            t0 = time.perf_counter()
            status = spmv.csr_transpose_gpu(AT, A.handle)
            t1 = time.perf_counter()
            stop.record()
            torch.cuda.synchronize()
            if status != 0:
                raise RuntimeError(spmv.spmv_error_string(status))
            spans.append(start.elapsed_time(stop))
            walls.append((t1 - t0) * 1e3)
            spmv.csr_destroy(AT)
        entry["build"] = {"span_ms": round(statistics.median(spans[1:]), 4),
                          "wall_ms": round(statistics.median(walls[1:]), 4),
                          "first_call_wall_ms": round(walls[0], 4)}

        AT = spmv.csr_create(0, 0, 0)
        assert spmv.csr_transpose_gpu(AT, A.handle) == 0
        x_rows = wl.vector_device(42, 1, A.rows)          # A^T x: x has num_rows entries
        x_cols = wl.vector_device(42, 2, A.cols)
        y_cols, y_rows = spmv.CudaBuffer(A.cols), spmv.CudaBuffer(A.rows)
        spmv_rows = {}
        for cname, (kt, tex) in CONFIGS.items():
            cfg = spmv.SpMVConfig(kt, 256, tex)
            t = median_ms(lambda: checked(spmv.spmv_csr_transpose(A.handle, x_rows, y_cols, cfg, A.rows)),
                          args.warmup, args.runs)
            e = median_ms(lambda: checked(spmv.spmv_csr(AT, x_rows, y_cols, cfg, A.rows)), args.warmup, args.runs)
            a = median_ms(lambda: checked(spmv.spmv_csr(A.handle, x_cols, y_rows, cfg, A.cols)), args.warmup,
                          args.runs)
            spmv_rows[cname] = {"spmv_csr_transpose_ms": round(t, 5), "spmv_csr_explicit_AT_ms": round(e, 5),
                                "spmv_csr_A_ms": round(a, 5), "transpose_over_explicit": round(t / e, 4)}
        entry["spmv"] = spmv_rows
        for b in (x_rows, x_cols, y_cols, y_rows):
            b.release()
        spmv.csr_destroy(AT)
        spmv.csr_invalidate_gpu_cache(A.handle)
        A.close()
        result["matrices"][name] = entry

    if args.merge_stats:
        result["kernel_stats"] = kernel_totals(args.merge_stats, args.builds + 3)   # (+ warm-up, explicit AT, cached)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
