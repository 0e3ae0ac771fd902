"""assemble_bench.py — csr_from_coo_gpu, csr_coo_refill and, on the same entry count in the same process,
csr_transpose_gpu.

Triplets are made in HBM with torch: `unique` random (row, column) cells of a square matrix, each repeated
`duplicates` times, in a random order, with normal values.  Shapes: C2 (1 M x 1 M, 16 M triplets, 4 per cell) and C5
(10 M x 10 M, 160 M triplets, 4 per cell); a cell drawn twice makes a longer run, so nnz_out is a little below
n / duplicates.  The key of both shapes is wider than 32 bits; `C2n` (60 K x 60 K, 16 M triplets) takes the 32-bit path.

* assembly: csr_from_coo_gpu into a fresh matrix, --builds times after one warm-up call; `span_ms` is the call's own
  device-event time (validation pass to the last kernel, the host's two reads and the allocations in between
  included), `wall_ms` the call's host time.
* refill: csr_coo_refill_async between two device events, median of --runs after --warmup; `stream_ms` is a plain
  device-to-device copy that reads and writes the refill's byte count (4 n order + 4 n values + 4 (nnz_out + 1) segment
  starts read, 4 nnz_out written), the same way.
* transpose: csr_transpose_gpu of a uniform matrix with the same number of entries, device-event span per build.
* host twin: csr_from_coo_cpu on the downloaded triplets (with the refill's values, which C holds by then), host wall
  time of one call, and whether the device matrix equals it bit for bit (--host; C5 needs about 6 GB of host memory
  and the better part of a minute).
* per kernel: from a `rocprofv3 --kernel-trace --stats` run of this tool (a run of its own: tracing slows the host):
  --merge-stats FILE adds calls and total time of every assemble_ and transpose_ kernel from its kernel_stats.csv, and
  the per-pass time and rate of the two scatter kernels over the bytes a pass moves: (key bytes + 4) read and written
  per entry for assemble_scatter_kernel, 12 read and 12 written for transpose_scatter_kernel.

    python tools/assemble_bench.py [--shapes C2,C5] [--builds 5] [--runs 20] [--warmup 5] [--host] [--out FILE]
                                   [--merge-stats CSV]
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

SHAPES = {"C2": (1_000_000, 4_000_000, 4), "C5": (10_000_000, 40_000_000, 4), "C2n": (60_000, 4_000_000, 4)}


def key_bytes(rows, cols):
    bits = max(rows - 1, 0).bit_length() + max(cols - 1, 0).bit_length()
    return 4 if bits <= 32 else 8


def kernel_totals(path):
    """{kernel: {calls, total_ms}} of the assemble_ and transpose_ kernels in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for family in ("assemble_", "transpose_"):
                if family in name:
                    short = family + name.split(family)[1].split("(")[0].split("<")[0]
                    entry = out.setdefault(short, {"calls": 0, "total_ms": 0.0})
                    entry["calls"] += int(row["Calls"])
                    entry["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="C2,C5")
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    spmv = importlib.import_module("gpu-spmv_amd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    stream = torch.cuda.current_stream().cuda_stream

    def event_ms(call, warmup, runs):
        times = []
        for i in range(warmup + runs):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(start.elapsed_time(stop))
        return statistics.median(times)

    result = {"tool": "tools/assemble_bench.py", "device": spmv.device_name(), "builds": args.builds,
              "runs": args.runs, "warmup": args.warmup,
              "statistic": "median; assembly span_ms: the call's device-event time, wall_ms: its host time; refill and "
                           "stream: device events around one enqueue; transpose: device events around the call",
              "shapes": {}}
    for name in args.shapes.split(","):
        size, unique, duplicates = SHAPES[name]
        n = unique * duplicates
        gen = torch.Generator(device="cuda")
        gen.manual_seed(42)
        cell_rows = torch.randint(0, size, (unique,), device="cuda", dtype=torch.int32, generator=gen)
        cell_cols = torch.randint(0, size, (unique,), device="cuda", dtype=torch.int32, generator=gen)
        order = torch.randperm(n, device="cuda", generator=gen)
        rows = cell_rows.repeat(duplicates)[order].contiguous()
        cols = cell_cols.repeat(duplicates)[order].contiguous()
        del cell_rows, cell_cols, order
        vals = torch.randn(n, device="cuda", dtype=torch.float32, generator=gen)
        vals2 = torch.randn(n, device="cuda", dtype=torch.float32, generator=gen)
        torch.cuda.synchronize()
        entry = {"rows": size, "cols": size, "triplets": n, "key_bytes": key_bytes(size, size)}

        spans, walls, res, plan, C = [], [], None, None, None
        for i in range(args.builds + 1):                  # the first build warms the allocator and the code objects
            if C is not None:
                spmv.coo_plan_destroy(plan)
                spmv.csr_destroy(C)
            C = spmv.csr_create(0, 0, 0)
            t0 = time.perf_counter()
            res, plan = spmv.csr_from_coo_gpu(C, size, size, n, rows.data_ptr(), cols.data_ptr(), vals.data_ptr(),
                                              want_plan=True)
            t1 = time.perf_counter()
            if res.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(res.error_code))
            spans.append(float(res.elapsed_ms))
            walls.append((t1 - t0) * 1e3)
        entry.update({"nnz_out": res.nnz_out, "combined": res.combined, "passes": res.passes,
                      "launches": res.launches, "tile_entries": res.tile_entries})
        entry["assembly"] = {"span_ms": round(statistics.median(spans[1:]), 4),
                             "wall_ms": round(statistics.median(walls[1:]), 4),
                             "first_call_wall_ms": round(walls[0], 4),
                             "triplets_per_s": round(n / (statistics.median(spans[1:]) * 1e-3), 0)}

        def refill():
            status = spmv.csr_coo_refill_async(plan, C, vals2.data_ptr(), stream=stream)
            if status != 0:
                raise RuntimeError(spmv.spmv_error_string(status))
        refill_ms = event_ms(refill, args.warmup, args.runs)
        refill_bytes = 4 * n + 4 * n + 4 * (res.nnz_out + 1) + 4 * res.nnz_out
        src = torch.empty(refill_bytes // 8, device="cuda", dtype=torch.float32)
        dst = torch.empty_like(src)
        stream_ms = event_ms(lambda: dst.copy_(src), args.warmup, args.runs)
        del src, dst
        entry["refill"] = {"ms": round(refill_ms, 4), "bytes": refill_bytes,
                           "gb_per_s": round(refill_bytes / (refill_ms * 1e-3) / 1e9, 1),
                           "stream_ms": round(stream_ms, 4), "refill_over_stream": round(refill_ms / stream_ms, 3)}

        if args.host:
            h_rows, h_cols, h_vals = rows.cpu().numpy(), cols.cpu().numpy(), vals2.cpu().numpy()     # C holds the refill
            H = spmv.csr_create(0, 0, 0)
            t0 = time.perf_counter()
            status = spmv.csr_from_coo_cpu(H, size, size, h_rows, h_cols, h_vals)
            t1 = time.perf_counter()
            assert status == 0 and H.contents.nnz == res.nnz_out
            # the bits, while both are at hand
            assert spmv.csr_from_gpu(C) == 0
            same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                       for a, b in zip(spmv.csr_host_arrays(C), spmv.csr_host_arrays(H)))
            entry["host_twin"] = {"wall_ms": round((t1 - t0) * 1e3, 1), "same_bits": bool(same),
                                  "over_device_wall": round((t1 - t0) * 1e3 / statistics.median(walls[1:]), 1)}
            spmv.csr_destroy(H)
            del h_rows, h_cols, h_vals
        spmv.coo_plan_destroy(plan)
        spmv.csr_destroy(C)
        del rows, cols, vals, vals2
        torch.cuda.empty_cache()

        # csr_transpose_gpu on the same entry count
        per_row = n // size if n // size >= 1 and size * (n // size) == n and n // size <= 64 else None
        if per_row is not None:
            A = wl.uniform_csr_device(42, size, size, per_row)
            spans = []
            for _ in range(args.builds + 1):
                AT = spmv.csr_create(0, 0, 0)
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                start.record()
                status = spmv.csr_transpose_gpu(AT, A.handle)
                stop.record()
                torch.cuda.synchronize()
                if status != 0:
                    raise RuntimeError(spmv.spmv_error_string(status))
                spans.append(start.elapsed_time(stop))
                spmv.csr_destroy(AT)
            digits = sum(1 for d in range(4) if ((size - 1) >> (8 * d)) & 255)
            entry["transpose"] = {"entries": A.nnz, "passes": digits, "span_ms": round(statistics.median(spans[1:]), 4)}
            A.close()
        result["shapes"][name] = entry

    if args.merge_stats:
        totals = kernel_totals(args.merge_stats)
        result["kernel_stats"] = totals
        builds = args.builds + 1
        scatter = {}
        new_bytes = sum(2 * (e["key_bytes"] + 4) * e["triplets"] * e["passes"] * builds
                        for e in result["shapes"].values())
        old_bytes = sum(24 * e["transpose"]["entries"] * e["transpose"]["passes"] * builds
                        for e in result["shapes"].values() if "transpose" in e)
        for kernel, moved in (("assemble_scatter_kernel", new_bytes), ("transpose_scatter_kernel", old_bytes)):
            if kernel in totals and totals[kernel]["total_ms"] > 0:
                scatter[kernel] = {"passes": totals[kernel]["calls"], "bytes_moved": moved,
                                   "total_ms": round(totals[kernel]["total_ms"], 3),
                                   "tb_per_s": round(moved / (totals[kernel]["total_ms"] * 1e-3) / 1e12, 3)}
        result["scatter"] = scatter
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
