"""csr_ops_bench.py — csr_add and csr_add_numeric on the device against the route that existed before them: the
re-assembly of both matrices' triplets with csr_from_coo_gpu.

Matrices are built in HBM by the device generators and normalised once (csr_row_indices_gpu + csr_from_coo_gpu, the
documented way to rows that are strictly ascending):

* C2_T    BASELINE config 2 (uniform 1 M x 1 M, 16 entries per row) plus its transpose (csr_transpose_gpu)
* C4_PAIR two power-law matrices of BASELINE config 4 (1 M rows, Pareto row lengths, max 10 000), seeds 42 and 43

Per case: the medians over --runs calls after --warmup of symbolic_ms and numeric_ms (device events inside csr_add;
allocation is outside both), the wall time of the whole call, the numeric_ms of csr_add_numeric alone, elapsed_ms of
csr_from_coo_gpu (summing mode) on A's triplets followed by B's, and the bytes the header says each pass must move
(4 B per entry of A and B for counting; 8 B per entry read plus 8 B per entry of C written for the numeric pass) with
the rates they give.  The triplets are concatenated through the host, outside every timed region.

    python tools/csr_ops_bench.py [--runs 10] [--warmup 2] [--cases C2_T,C4_PAIR] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="C2_T,C4_PAIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_ops_bench.json"))
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    lib = spmv.lib()

    def checked(res):
        if res.error_code != 0:
            raise RuntimeError(spmv.spmv_error_string(res.error_code))
        return res

    def triplets(M):
        """(rows, cols, vals) of a device matrix, on the host"""
        m = M.contents
        d_rows = spmv.CudaBuffer(max(m.nnz, 1), "int32")
        if spmv.csr_row_indices_gpu(M, d_rows) != 0:
            raise RuntimeError("csr_row_indices_gpu failed")
        rows = d_rows.copyToHost(m.nnz)
        d_rows.release()
        cols, vals = np.empty(m.nnz, np.int32), np.empty(m.nnz, np.float32)
        lib.spmv_c_memcpy_d2h(cols.ctypes.data, m.d_col_indices, 4 * m.nnz)
        lib.spmv_c_memcpy_d2h(vals.ctypes.data, m.d_values, 4 * m.nnz)
        return rows, cols, vals

    def assembled(num_rows, num_cols, parts, timed_runs=0):
        """csr_from_coo_gpu (summing mode) of the concatenated triplets: (matrix, elapsed_ms of each timed run)"""
        rows, cols, vals = (np.concatenate([p[i] for p in parts]) for i in range(3))
        bufs = [spmv.CudaBuffer(rows.size, "int32"), spmv.CudaBuffer(rows.size, "int32"), spmv.CudaBuffer(rows.size)]
        for buf, host in zip(bufs, (rows, cols, vals)):
            buf.copyFromHost(host, host.size)
        C = spmv.csr_create(0, 0, 0)
        times = []
        for i in range(args.warmup + timed_runs if timed_runs else 1):
            res = checked(spmv.csr_from_coo_gpu(C, num_rows, num_cols, rows.size, *bufs))
            if timed_runs and i >= args.warmup:
                times.append(res.elapsed_ms)
        for buf in bufs:
            buf.release()
        return C, times

    def normalised(handle):
        m = handle.contents
        return assembled(m.num_rows, m.num_cols, [triplets(handle)])[0]

    def operands(name):
        n = 1_000_000
        if name == "C2_T":
            raw = wl.uniform_csr_device(42, n, n, 16)
            A = normalised(raw.handle)
            raw.close()
            B = spmv.csr_create(0, 0, 0)
            if spmv.csr_transpose_gpu(B, A) != 0:
                raise RuntimeError("csr_transpose_gpu failed")
            return A, B
        out = []
        for seed in (42, 43):
            raw = wl.power_law_csr_device(seed, n, n)
            out.append(normalised(raw.handle))
            raw.close()
        return tuple(out)

    result = {"tool": "tools/csr_ops_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "statistic": "median of the runs after the warm-up calls", "cases": {}}
    for name in args.cases.split(","):
        A, B = operands(name)
        sym, num, wall, refill = [], [], [], []
        C = spmv.csr_create(0, 0, 0)
        for i in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            res = checked(spmv.csr_add(C, 1.0, A, 0.5, B))
            t1 = time.perf_counter()
            if i >= args.warmup:
                sym.append(res.symbolic_ms)
                num.append(res.numeric_ms)
                wall.append((t1 - t0) * 1e3)
        for i in range(args.warmup + args.runs):
            again = checked(spmv.csr_add_numeric(C, 1.0, A, 0.25, B))
            if i >= args.warmup:
                refill.append(again.numeric_ms)
        m = A.contents
        T, route = assembled(m.num_rows, m.num_cols, [triplets(A), triplets(B)], timed_runs=args.runs)
        if T.contents.nnz != res.nnz:
            raise RuntimeError("the two routes disagree on nnz(C)")
        s, nm, rf = statistics.median(sym), statistics.median(num), statistics.median(refill)
        entries = m.nnz + B.contents.nnz
        count_bytes, numeric_bytes = 4 * entries, 8 * entries + 8 * res.nnz
        entry = {"rows": m.num_rows, "cols": m.num_cols, "nnz_A": m.nnz, "nnz_B": B.contents.nnz, "nnz_C": res.nnz,
                 "common": res.common, "max_row_nnz": res.max_row_nnz, "lanes": res.lanes, "launches": res.launches,
                 "symbolic_ms": round(s, 4), "numeric_ms": round(nm, 4), "call_wall_ms": round(statistics.median(wall), 4),
                 "numeric_alone_ms": round(rf, 4), "triplet_route_ms": round(statistics.median(route), 4),
                 "count_bytes": count_bytes, "numeric_bytes": numeric_bytes,
                 "count_GBps": round(count_bytes / (s * 1e6), 1) if s > 0 else None,
                 "numeric_GBps": round(numeric_bytes / (nm * 1e6), 1) if nm > 0 else None,
                 "numeric_alone_GBps": round(numeric_bytes / (rf * 1e6), 1) if rf > 0 else None}
        for M in (A, B, C, T):
            spmv.csr_destroy(M)
        result["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
