"""eigs_bench.py — eigs_sym beside gmres_solve on the same matrices: what a Lanczos step at full basis costs beside
the GMRES step that moves the same bytes through the same three basis kernels, and what the thick restart's rotation
costs beside a plain device copy of the bytes it reads and writes.

Matrices (numpy, gpu-spmv_amd/spd.py): poisson2d(m2) and poisson3d(m3), the sizes of tools/gmres_bench.py.  Per matrix,
engine 0, median of --runs after one warm-up:
* eigs_sym to 1e-5, k LARGEST values with a basis of m: steps, restarts, converged, max_residual, elapsed_ms.
* the Lanczos step at j = m - 1: elapsed_ms of a call capped at m steps less one capped at m - 1 (tolerance 0; both
  pay one close and one finish, so the difference is the step alone).
* the GMRES step at j = m - 1 by DESIGN.md section 4.14's method: gmres_solve (restart m, NONE, tolerance 0) capped
  at m steps less one capped at m - 1.  A Lanczos step should cost no more than that plus 10 %.
* a cycle: (elapsed_ms of a call capped at 2m - p steps) less (one capped at m): m - p steps plus one close with its
  Jacobi sweeps and its rotation, p = k + (m - k) / 2; less (m - p) full-basis steps it bounds the close from below.
  Beside it a torch device-to-device copy moving the rotation's bytes: m + 1 vectors read, p + 1 written.

    python tools/eigs_bench.py [--m2 512] [--m3 96] [--k 8] [--basis 30] [--runs 3] [--out FILE]
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
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--basis", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=3000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    import torch

    k, m = args.k, args.basis
    p = min(k + (m - k) // 2, m - 1)
    makers = {f"poisson2d({args.m2})": lambda: spd.poisson2d(args.m2),
              f"poisson3d({args.m3})": lambda: spd.poisson3d(args.m3)}
    result = {"tool": "tools/eigs_bench.py", "device": spmv.device_name(), "k": k, "basis": m, "kept": p,
              "runs": args.runs, "statistic": "median over runs after one warm-up; engine 0; LARGEST", "matrices": {}}
    for name, make in makers.items():
        n, rp, ci, va = make()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        values, residuals, vectors = spmv.CudaBuffer(k), spmv.CudaBuffer(k), spmv.CudaBuffer(k * n)
        b, x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32), n)
        zeros = np.zeros(n, np.float32)

        def timed(call):
            runs = []
            for run in range(args.runs + 1):
                res = call()
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run:
                    runs.append(res)
            runs.sort(key=lambda r: r.elapsed_ms)
            return runs[len(runs) // 2]

        def eigs(tolerance, cap):
            cfg = spmv.EigsConfig(num_values=k, which=0, basis=m, tolerance=tolerance, max_iterations=cap, engine=0)
            return timed(lambda: spmv.eigs_sym(A, values, vectors, n, residuals, None, cfg))

        def gmres(cap):
            cfg = spmv.GMRESConfig(tolerance=0.0, max_iterations=cap, restart=m, preconditioner=0, engine=0)

            def call():
                x.copyFromHost(zeros, n)
                return spmv.gmres_solve(A, b, x, cfg)
            return timed(call)

        full = eigs(1e-5, args.max_iterations)
        entry = {"rows": n, "nnz": int(ci.size),
                 "eigs_sym": {"steps": full.iterations, "restarts": full.restarts, "converged": full.converged,
                              "max_residual": full.max_residual, "elapsed_ms": round(full.elapsed_ms, 3)}}
        e_m, e_m1 = eigs(0.0, m).elapsed_ms, eigs(0.0, m - 1).elapsed_ms
        g_m, g_m1 = gmres(m).elapsed_ms, gmres(m - 1).elapsed_ms
        e_cycle = eigs(0.0, 2 * m - p).elapsed_ms
        entry["last_column"] = {"j": m - 1, "lanczos_step_ms": round(e_m - e_m1, 4),
                                "gmres_step_ms": round(g_m - g_m1, 4),
                                "ratio": round((e_m - e_m1) / (g_m - g_m1), 3) if g_m > g_m1 else None}
        copy_bytes = (m + 1 + p + 1) * 4 * n
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
        entry["restart"] = {"steps_after": m - p, "cycle_ms": round(e_cycle - e_m, 4),
                            "close_ms_less_full_steps": round(e_cycle - e_m - (m - p) * (e_m - e_m1), 4),
                            "rotation_model_bytes": copy_bytes,
                            "device_copy_same_bytes_ms": round(statistics.median(times), 4)}
        del src, dst
        for buf in (values, residuals, vectors, b, x):
            buf.release()
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
