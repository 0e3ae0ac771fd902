"""sptrsv_analysis_bench.py — the level analysis on the host against the level analysis on the device (DESIGN.md
§4.23), on the three matrices of tools/sptrsv_bench.py.

Matrices (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu):
* P3D: the 7-point 3-D Poisson matrix at 160^3 (4.1 M rows; 478 levels, wide in the middle);
* RSPD: the random SPD matrix S + S^T + D at 4 M rows and 7 + 7 + 1 entries per row;
* P2D64: the 5-point 2-D Poisson matrix at 64^2 (127 levels of at most 64 rows).

Per matrix, LOWER and UPPER: --runs times csr_invalidate_gpu_cache + sptrsv_analyze, then the same with
sptrsv_analyze_device; analysis_ms is the wall time the call reports for its build (read-back or kernels, grouping,
upload or the level-pointer download).  Reported: every run's analysis_ms and the median for both; levels and launches
(equal for both by construction: checked); the arrays compared int for int; and the rounds the device analysis
enqueues, restated here from the level widths: a round is one pair of launches (a single-workgroup run of narrow
levels, one wide level), rounds are enqueued in batches of 8, and the host looks at the state one batch behind.

    python tools/sptrsv_analysis_bench.py [--matrices P3D,RSPD,P2D64] [--runs 3] [--out FILE]
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

NARROW, MAX_RUN_LEVELS, ROUNDS_PER_BATCH = 256, 8192, 8       # csrc/internal.h, csrc/solver_common.h


def rounds_needed(widths) -> int:
    """pairs of launches until the single-workgroup launch finds the empty frontier"""
    levels, r, pairs = len(widths), 0, 0
    while True:
        pairs += 1
        walked = 0
        while r < levels and widths[r] <= NARROW and walked < MAX_RUN_LEVELS:
            r += 1
            walked += 1
        if r == levels:
            return pairs
        if r < levels and widths[r] > NARROW:
            r += 1                                               # the wide launch of this pair


def rounds_enqueued(widths, n) -> int:
    """what the host loop enqueues: a batch more than the one that held the last needed round, at most n + 1"""
    needed = rounds_needed(widths)
    batches = -(-needed // ROUNDS_PER_BATCH) + 1
    return min(batches * ROUNDS_PER_BATCH, n + 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="P3D,RSPD,P2D64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    makers = {"P3D": lambda: spd.poisson3d(160), "RSPD": lambda: spd.random_spd(4_000_000, 7, seed=42),
              "P2D64": lambda: spd.poisson2d(64)}
    result = {"tool": "tools/sptrsv_analysis_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "statistic": "analysis_ms of sptrsv_analyze / sptrsv_analyze_device after csr_invalidate_gpu_cache: "
                           "every run and the median",
              "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        entry = {"rows": n, "nnz": int(ci.size), "structure_bytes_read_back_by_the_host_analysis": 4 * (n + 1 + int(ci.size)),
                 "triangles": {}}
        for uplo in (0, 1):
            timings, schedules = {}, {}
            for origin, analyze in (("host", spmv.sptrsv_analyze), ("device", spmv.sptrsv_analyze_device)):
                times = []
                for _ in range(args.runs):
                    spmv.csr_invalidate_gpu_cache(A)
                    res = analyze(A, uplo)
                    if res.error_code != 0:
                        raise RuntimeError(spmv.spmv_error_string(res.error_code))
                    times.append(float(res.analysis_ms))
                timings[origin] = times
                status, level_ptr, order, info = spmv.sptrsv_schedule_get(A, uplo)
                assert status == 0 and info.built_on_device == (origin == "device")
                schedules[origin] = (level_ptr, order, info.num_levels, info.launches, info.triangle_nnz)
            host, device = schedules["host"], schedules["device"]
            same = bool(np.array_equal(host[0], device[0]) and np.array_equal(host[1], device[1]) and
                        host[2:] == device[2:])
            widths = np.diff(device[0]).tolist()
            entry["triangles"]["upper" if uplo else "lower"] = {
                "num_levels": device[2], "launches": device[3], "triangle_nnz": int(device[4]),
                "widest_level": int(max(widths)), "rounds_needed": rounds_needed(widths),
                "rounds_enqueued": rounds_enqueued(widths, n), "device_equals_host": same,
                "host_analysis_ms": [round(t, 3) for t in timings["host"]],
                "device_analysis_ms": [round(t, 3) for t in timings["device"]],
                "host_median_ms": round(statistics.median(timings["host"]), 3),
                "device_median_ms": round(statistics.median(timings["device"]), 3),
                "host_over_device": round(statistics.median(timings["host"]) /
                                          max(statistics.median(timings["device"]), 1e-9), 2)}
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
