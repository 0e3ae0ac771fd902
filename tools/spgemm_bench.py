"""spgemm_bench.py — spgemm_csr and spgemm_csr_numeric on the device against spgemm_cpu_csr on one host thread.

Matrices are built in HBM by the device generators:

* AA_C2   A·A for BASELINE config 2 (uniform 1 M x 1 M, 16 entries per row)
* AA_C4   A·A for the power-law config 4 (1 M rows, max 10 000): its hub rows reach the dense class
* ATA     A^T·A for a uniform 1 M x 64 K matrix with 16 entries per row, A^T from csr_transpose_gpu

Per case: the medians over --runs calls after --warmup of symbolic_ms and numeric_ms (device events inside
spgemm_csr; validation and allocation are outside both), the wall time of the whole call, the numeric_ms of
spgemm_csr_numeric alone, products per second (products / (symbolic_ms + numeric_ms)), nnz(C) and the class
histograms of both passes.  --host adds spgemm_cpu_csr on the same inputs (one run: it takes seconds).

The comparison with rocSPARSE's rocsparse_spgemm on the same device arrays is NOT implemented: the field
"rocsparse_spgemm_ms" is a placeholder that is always null.

    python tools/spgemm_bench.py [--runs 10] [--warmup 2] [--cases AA_C2,AA_C4,ATA] [--host] [--out FILE]
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
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="AA_C2,AA_C4,ATA")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_bench.json"))
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()

    def checked(res):
        if res.error_code != 0:
            raise RuntimeError(spmv.spmv_error_string(res.error_code))
        return res

    def operands(name):
        """(left handle, right handle, things to close)"""
        if name == "AA_C2":
            A = wl.uniform_csr_device(42, 1_000_000, 1_000_000, 16)
            return A.handle, A.handle, [A]
        if name == "AA_C4":
            A = wl.power_law_csr_device(42, 1_000_000, 1_000_000)
            return A.handle, A.handle, [A]
        A = wl.uniform_csr_device(42, 1_000_000, 65_536, 16)
        AT = spmv.csr_create(0, 0, 0)
        if spmv.csr_transpose_gpu(AT, A.handle) != 0:
            raise RuntimeError("csr_transpose_gpu failed")
        return AT, A.handle, [A, AT]

    result = {"tool": "tools/spgemm_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "statistic": "median of the runs after the warm-up calls", "cases": {}}
    for name in args.cases.split(","):
        L, R, held = operands(name)
        sym, num, wall = [], [], []
        C = spmv.csr_create(0, 0, 0)
        for i in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            res = checked(spmv.spgemm_csr(C, L, R))
            t1 = time.perf_counter()
            if i >= args.warmup:
                sym.append(res.symbolic_ms)
                num.append(res.numeric_ms)
                wall.append((t1 - t0) * 1e3)
        refill = []
        for i in range(args.warmup + args.runs):
            again = checked(spmv.spgemm_csr_numeric(C, L, R))
            if i >= args.warmup:
                refill.append(again.numeric_ms)
        s, n = statistics.median(sym), statistics.median(num)
        entry = {"rows": L.contents.num_rows, "inner": L.contents.num_cols, "cols": R.contents.num_cols,
                 "nnz_left": L.contents.nnz, "nnz_right": R.contents.nnz, "nnz_C": res.nnz,
                 "products": res.products, "max_row_products": res.max_row_products, "max_row_nnz": res.max_row_nnz,
                 "lanes": res.lanes, "symbolic_rows": list(res.symbolic_rows), "numeric_rows": list(res.numeric_rows),
                 "symbolic_ms": round(s, 4), "numeric_ms": round(n, 4), "call_wall_ms": round(statistics.median(wall), 4),
                 "numeric_alone_ms": round(statistics.median(refill), 4),
                 "products_per_s": round(res.products / ((s + n) * 1e-3), 1) if s + n > 0 else None,
                 "rocsparse_spgemm_ms": None}
        if args.host:
            hosts = []
            for M in (L, R):
                H = spmv.csr_create(M.contents.num_rows, M.contents.num_cols, M.contents.nnz)
                m = H.contents
                lib = spmv.lib()
                lib.spmv_c_memcpy_d2h(m.row_ptrs, M.contents.d_row_ptrs, 4 * (m.num_rows + 1))
                lib.spmv_c_memcpy_d2h(m.col_indices, M.contents.d_col_indices, 4 * m.nnz)
                lib.spmv_c_memcpy_d2h(m.values, M.contents.d_values, 4 * m.nnz)
                hosts.append(H)
            HC = spmv.csr_create(0, 0, 0)
            t0 = time.perf_counter()
            status = spmv.spgemm_cpu_csr(HC, hosts[0], hosts[1])
            entry["host_one_thread_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert status == 0 and HC.contents.nnz == res.nnz
            for H in hosts + [HC]:
                spmv.csr_destroy(H)
        spmv.csr_destroy(C)
        for h in held:
            h.close() if hasattr(h, "close") else spmv.csr_destroy(h)
        result["cases"][name] = entry
        print(json.dumps({name: entry}), flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
