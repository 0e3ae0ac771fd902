"""minres_bench.py — minres_solve time per step against cg_solve on the same matrix, and the launches per step.

Matrix (numpy, gpu-spmv_amd/spd.py, uploaded with csr_from_arrays + csr_to_gpu): P3D128, the 7-point Laplacian at 128^3
(2.1 M rows, 14.6 M entries).  cg_solve solves it as it is; minres_solve solves it as it is (the time per step does
not depend on the shift) and, for the converging solve, shifted between its 4th and 5th distinct eigenvalue.  P2D64
(2-D Laplacian at 64^2), where the launch latency dominates: reported only.

Per solver: --runs solves of exactly --iters steps (tolerance 0, engine 0) after one warm-up solve; ms per step =
median elapsed_ms / iters (minres_solve's elapsed_ms includes its one recomputed-residual launch: 1 / iters of a step).
Solvers: cg (NONE), minres (NONE), minres_jacobi, minres_ic (F = ic0_csr of the matrix).  The byte model of a step:
  cg      NONE  8 nnz + 11 * 4 n   SpMV + dot: p gathered, q out 8 | update: p, q, x, r in, x, r out 24 | direction:
                r, p in, p out 12; JACOBI adds dinv twice
  minres  NONE  8 nnz + 14 * 4 n   SpMV + dot: v gathered, r1 in, y out 12 | Lanczos: y, r2 in, y out 12 | update:
                y, v, w_k-2, w_k-1, x in, w, x, v out 32; JACOBI adds dinv twice: 16 * 4 n
(the row's own entry of the gathered vector comes from the cache in both)
so the predicted ratio minres / cg with NONE is (8 nnz + 56 n) / (8 nnz + 44 n), 1.12 on a 7-point stencil, and
(8 nnz + 64 n) / (8 nnz + 44 n) = 1.2 for minres JACOBI against cg NONE.  The run-to-run spread of each figure is
reported beside it (max - min over the runs, relative to the median).

--only SOLVER runs that solver alone, --runs 1 --iters N: the form to count launches per step from a
`rocprofv3 --kernel-trace --stats` run (calls of each kernel / N); --merge-stats SOLVER=CSV adds such a run's
per-kernel split to the output.

    python tools/minres_bench.py [--matrices P3D128,P2D64] [--iters 100] [--runs 5] [--only minres] [--out FILE]
                                 [--merge-stats minres=a.csv,minres_ic=b.csv]
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

from cg_bench import kernel_split  # noqa: E402

SOLVERS = ("cg", "minres", "minres_jacobi", "minres_ic")
VECTOR_WORDS_PER_ROW = {"cg": 11, "minres": 14, "minres_jacobi": 16}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="P3D128,P2D64")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", default=None, choices=SOLVERS)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", default=None)
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    makers = {"P3D128": (lambda: spd.poisson3d(128), 128, 3), "P2D64": (lambda: spd.poisson2d(64), 64, 2)}
    result = {"tool": "tools/minres_bench.py", "device": spmv.device_name(), "iters": args.iters, "runs": args.runs,
              "statistic": "median over runs; ms_per_step = elapsed_ms / iters (tolerance 0, engine 0); spread = "
                           "(max - min) / median over the runs",
              "launches_per_step": {"cg": 3, "minres": 3, "minres_jacobi": 3,
                                    "minres_ic": "4 + launches(LOWER) + launches(UPPER)"},
              "matrices": {}}
    for name in args.matrices.split(","):
        maker, m, dims = makers[name]
        n, rp, ci, va = maker()
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        b = spmv.CudaBuffer(n)
        b.copyFromHost(np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32), n)
        x = spmv.CudaBuffer(n)
        zeros = np.zeros(n, np.float32)
        d_l = spmv.CudaBuffer(nnz)
        fact = spmv.ic0_csr(A, d_l)
        assert fact.error_code == 0 and fact.bad_pivot == -1
        F = spmv.csr_wrap_device(n, n, nnz, A.contents.d_row_ptrs, A.contents.d_col_indices, d_l.get())
        model = {k: 8 * nnz + 4 * w * n for k, w in VECTOR_WORDS_PER_ROW.items()}
        entry = {"rows": n, "nnz": nnz, "bytes_model": model,
                 "predicted_ratio": {"minres_over_cg": round(model["minres"] / model["cg"], 4),
                                     "minres_jacobi_over_cg": round(model["minres_jacobi"] / model["cg"], 4)},
                 "solvers": {}}

        def solve(kind, tol, cap, shift=0.0):
            x.copyFromHost(zeros, n)
            if kind == "cg":
                return spmv.cg_solve(A, b, x, spmv.CGConfig(tolerance=tol, max_iterations=cap, preconditioner=0,
                                                            engine=0))
            cfg = spmv.MinresConfig(tolerance=tol, max_iterations=cap, engine=0, shift=shift,
                                    preconditioner=1 if kind == "minres_jacobi" else 0)
            if kind == "minres_ic":
                return spmv.minres_solve_ic(A, F, b, x, cfg)
            return spmv.minres_solve(A, b, x, cfg)

        for kind in SOLVERS:
            if args.only and kind != args.only:
                continue
            times, res = [], None
            for run in range(args.runs + 1):
                res = solve(kind, 0.0, args.iters)
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                if run or args.runs == 1:
                    times.append(res.elapsed_ms / max(res.iterations, 1))
            med = statistics.median(times)
            entry["solvers"][kind] = {"ms_per_step": round(med, 5), "iterations_run": res.iterations,
                                      "breakdown": res.breakdown,
                                      "spread": round((max(times) - min(times)) / med, 4),
                                      "model_tb_s": round(model[kind] / (med * 1e-3) / 1e12, 3) if kind in model
                                      else None}
        got = entry["solvers"]
        if "cg" in got and "minres" in got:
            entry["measured_ratio"] = {
                "minres_over_cg": round(got["minres"]["ms_per_step"] / got["cg"]["ms_per_step"], 4),
                "minres_jacobi_over_cg": round(got["minres_jacobi"]["ms_per_step"] / got["cg"]["ms_per_step"], 4)}
        if not args.only:
            # a converging indefinite solve: the shift halfway between the 4th and 5th distinct eigenvalue
            c = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
            lam = c
            for _ in range(dims - 1):
                lam = np.unique(np.round((lam[:, None] + c[None, :]).ravel(), 12))[:64]
            shift = float(np.float32(0.5 * (lam[3] + lam[4])))
            entry["converge_shifted_1e-5"] = {"shift": shift}
            for kind in ("minres", "minres_jacobi", "minres_ic"):
                res = solve(kind, 1e-5, 3000, shift)
                entry["converge_shifted_1e-5"][kind] = {
                    "iterations": res.iterations, "converged": res.converged, "breakdown": res.breakdown,
                    "relative_residual": res.relative_residual,
                    "true_relative_residual": res.true_relative_residual, "elapsed_ms": round(res.elapsed_ms, 3)}
        spmv.csr_destroy(F)
        for buf in (b, x, d_l):
            buf.release()
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    for pair in filter(None, (args.merge_stats or "").split(",")):
        kind, path = pair.split("=", 1)
        result.setdefault("kernel_stats", {})[kind] = kernel_split(path)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
