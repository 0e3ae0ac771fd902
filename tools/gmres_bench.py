"""gmres_bench.py — gmres_solve / gmres_solve_lu beside bicgstab_solve / bicgstab_solve_lu to 1e-6, and the cost of
the orthogonalisation at the last column of a cycle beside a plain device copy of the same byte count.

Matrices (numpy, gpu-spmv_amd/nonsym.py): convdiff2d(m2) and convdiff3d(m3) at a mild (1) and a strong (50) wind.
Per matrix, engine 0, x0 = 0, median of --runs after one warm-up:
* NONE, JACOBI and ILU(0) (ilu0_csr's factor wrapped over A's structure): steps, restarts, elapsed_ms, converged and
  the reported residual of gmres_solve* (--restart), beside iterations, elapsed_ms, converged, breakdown of
  bicgstab_solve*.  A BiCGSTAB iteration holds two SpMVs, a GMRES step one.
* the step at j = restart - 1 (NONE): elapsed_ms of a solve capped at `restart` steps less one capped at
  `restart - 1` (tolerance 0; the first also pays the cycle's close), less one spmv_csr: what the three basis kernels,
  gmres_hessenberg and the close cost there.  Beside it a torch device-to-device copy moving the bytes the three
  kernels read and write: 4 passes over the `restart` basis vectors (gmres_update_multidot reads them twice) and
  5 reads + 2 writes of w, 4 bytes each per row.

    python tools/gmres_bench.py [--m2 512] [--m3 96] [--restart 30] [--runs 3] [--out FILE]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--m2", type=int, default=512)
    ap.add_argument("--m3", type=int, default=96)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    nonsym = importlib.import_module("gpu-spmv_amd.nonsym")
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    import torch

    m = args.restart
    makers = {f"convdiff2d({args.m2},{w})": (lambda w=w: nonsym.convdiff2d(args.m2, float(w))) for w in (1, 50)}
    makers.update({f"convdiff3d({args.m3},{w})": (lambda w=w: nonsym.convdiff3d(args.m3, float(w))) for w in (1, 50)})
    result = {"tool": "tools/gmres_bench.py", "device": spmv.device_name(), "restart": m, "runs": args.runs,
              "statistic": "median over runs after one warm-up; engine 0; x0 = 0; tolerance 1e-6", "matrices": {}}
    for name, make in makers.items():
        n, rp, ci, va = make()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        b, x, y = spmv.CudaBuffer(n), spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32), n)
        zeros = np.zeros(n, np.float32)
        d_lu = spmv.CudaBuffer(ci.size)
        assert spmv.ilu0_csr(A, d_lu).error_code == 0
        F = spmv.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, d_lu.get())

        def timed(call):
            runs = []
            for run in range(args.runs + 1):
                x.copyFromHost(zeros, n)
                res = call()
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run:
                    runs.append(res)
            runs.sort(key=lambda r: r.elapsed_ms)
            return runs[len(runs) // 2]

        entry = {"rows": n, "nnz": int(ci.size), "preconditioners": {}}
        for label, pre in (("none", 0), ("jacobi", 1), ("ilu0", None)):
            gcfg = spmv.GMRESConfig(tolerance=1e-6, max_iterations=args.max_iterations, restart=m,
                                    preconditioner=pre or 0, engine=0)
            bcfg = spmv.BiCGStabConfig(tolerance=1e-6, max_iterations=args.max_iterations, preconditioner=pre or 0,
                                       engine=0)
            if pre is None:
                g = timed(lambda: spmv.gmres_solve_lu(A, F, b, x, gcfg))
                s = timed(lambda: spmv.bicgstab_solve_lu(A, F, b, x, bcfg))
            else:
                g = timed(lambda: spmv.gmres_solve(A, b, x, gcfg))
                s = timed(lambda: spmv.bicgstab_solve(A, b, x, bcfg))
            entry["preconditioners"][label] = {
                "gmres": {"steps": g.iterations, "restarts": g.restarts, "elapsed_ms": round(g.elapsed_ms, 3),
                          "converged": g.converged, "breakdown": g.breakdown,
                          "relative_residual": g.relative_residual},
                "bicgstab": {"iterations": s.iterations, "elapsed_ms": round(s.elapsed_ms, 3),
                             "converged": s.converged, "breakdown": s.breakdown,
                             "relative_residual": s.relative_residual}}
        # the step at j = restart - 1
        cap = lambda k: spmv.GMRESConfig(tolerance=0.0, max_iterations=k, restart=m, preconditioner=0, engine=0)
        full = timed(lambda: spmv.gmres_solve(A, b, x, cap(m))).elapsed_ms
        less = timed(lambda: spmv.gmres_solve(A, b, x, cap(m - 1))).elapsed_ms if m > 1 else 0.0
        t_spmv = statistics.median(wl.time_spmv_csr(A, b, y, 1, warmup=5, runs=20))
        copy_bytes = (4 * m + 7) * 4 * n
        src = torch.empty(copy_bytes // 2, dtype=torch.uint8, device="cuda")     # a copy moves its size twice
        dst = torch.empty_like(src)
        times = []
        for run in range(args.runs + 2):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            dst.copy_(src)
            stop.record()
            stop.synchronize()
            if run >= 2:
                times.append(start.elapsed_time(stop))
        entry["last_column"] = {"j": m - 1, "step_ms": round(full - less, 4), "spmv_csr_ms": round(t_spmv, 4),
                                "step_less_spmv_ms": round(full - less - t_spmv, 4),
                                "model_bytes": copy_bytes, "device_copy_same_bytes_ms": round(statistics.median(times), 4)}
        del src, dst
        spmv.csr_destroy(F)
        for buf in (b, x, y, d_lu):
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
