"""multicolor_bench.py — natural against multicoloured ordering for the triangular solves, IC(0) and cg_solve_ic.

On poisson3d(160) and poisson2d(512) (gpu-spmv_amd/spd.py), in one process:

* reorder: colours and rounds of csr_color with its device time; the time of color_ordering and of csr_permute_gpu
  (host wall time of the synchronous calls, the median of --runs), the latter beside a device-to-device copy of the
  bytes it moves (column indices and values, read once and written once);
* per ordering (natural = the matrix as generated, coloured = B = P A P^T): sptrsv_csr launches and elapsed_ms for
  both triangles, ic0_csr's elapsed_ms, and cg_solve_ic to 1e-6: iterations, ms per step and ms to solution, against
  cg_solve with the Jacobi preconditioner on the same system (the right-hand side is permuted with permute_gather for
  the coloured solve); every solve has the default cap of 1000 steps, and `converged` says whether it got there.  Every device time is the library's own elapsed_ms, the median of --runs after one warm-up.

    python tools/multicolor_bench.py [--runs 5] [--matrices poisson3d(160),poisson2d(512)] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL = 1e-6
JACOBI = 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--matrices", default="poisson3d(160),poisson2d(512)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    def note(*what):
        print("[multicolor_bench]", *what, file=sys.stderr, flush=True)

    def ok(res):
        if res.error_code != 0:
            raise RuntimeError(spmv.spmv_error_string(res.error_code))
        return res

    def median_of(call):
        call()
        return statistics.median(call() for _ in range(args.runs))

    def wall_ms(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        status = call()
        t1 = time.perf_counter()
        if status != 0:
            raise RuntimeError(spmv.spmv_error_string(status))
        return (t1 - t0) * 1e3

    def ordering_figures(M, n, nnz, d_b, d_x):
        """the triangular solves, the factorisation and the two solvers on the device matrix M"""
        out = {}
        for name, uplo in (("lower", 0), ("upper", 1)):
            analysis = ok(spmv.sptrsv_analyze(M, uplo))
            cfg = spmv.SpTRSVConfig(uplo=uplo)
            ms = median_of(lambda: float(ok(spmv.sptrsv_csr(M, d_b, d_x, cfg)).elapsed_ms))
            out["sptrsv_" + name] = {"levels": analysis.num_levels, "launches": analysis.launches,
                                     "analysis_ms": round(float(analysis.analysis_ms), 3), "elapsed_ms": round(ms, 4)}
        d_l = spmv.CudaBuffer(nnz)
        out["ic0_ms"] = round(median_of(lambda: float(ok(spmv.ic0_csr(M, d_l)).elapsed_ms)), 4)
        F = spmv.csr_wrap_device(n, n, nnz, M.contents.d_row_ptrs, M.contents.d_col_indices, d_l.get())
        zeros = np.zeros(n, np.float32)

        def solve(call):
            d_x.copyFromHost(zeros, n)
            return ok(call())
        for name, call in (("cg_ic", lambda: spmv.cg_solve_ic(M, F, d_b, d_x, spmv.CGConfig(tolerance=TOL))),
                           ("cg_jacobi", lambda: spmv.cg_solve(M, d_b, d_x, spmv.CGConfig(tolerance=TOL,
                                                                                         preconditioner=JACOBI)))):
            solve(call)
            runs = [solve(call) for _ in range(args.runs)]
            ms = statistics.median(float(r.elapsed_ms) for r in runs)
            its = runs[-1].iterations
            out[name] = {"iterations": its, "converged": int(runs[-1].converged),
                         "relative_residual": float(runs[-1].relative_residual), "ms_per_step": round(ms / max(its, 1), 5),
                         "ms_to_solution": round(ms, 3)}
        spmv.csr_destroy(F)
        d_l.release()
        return out

    result = {"tool": "tools/multicolor_bench.py", "device": spmv.device_name(), "runs": args.runs, "tolerance": TOL,
              "statistic": "median of runs after one warm-up; device times are the library's elapsed_ms, "
                           "color_ordering / csr_permute_gpu host wall time of the synchronous call",
              "matrices": {}}
    for name in args.matrices.split(","):
        kind, size = re.fullmatch(r"(poisson[23]d)\((\d+)\)", name.strip()).groups()
        n, rp, ci, va = getattr(spd, kind)(int(size))
        nnz = int(ci.size)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        if spmv.csr_to_gpu(A) != 0:
            raise RuntimeError("csr_to_gpu failed")
        entry = {"rows": n, "nnz": nnz}
        note(name, "on the device:", n, "rows,", nnz, "entries")
        b = np.random.default_rng(1).uniform(-1.0, 1.0, n).astype(np.float32)
        d_b, d_pb, d_x = spmv.CudaBuffer(n), spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        d_b.copyFromHost(b, n)

        # ---- the reordering, step by step and then in one call ----
        d_colors, d_perm, d_inverse = (spmv.CudaBuffer(n, "int32") for _ in range(3))
        colour_runs = [ok(spmv.csr_color(A, d_colors)) for _ in range(args.runs + 1)][1:]
        colour = colour_runs[-1]
        promised = ok(spmv.csr_color(A, d_colors, spmv.ColorConfig(symmetric_pattern=1)))
        promised_ms = median_of(lambda: float(ok(spmv.csr_color(A, d_colors,
                                                                spmv.ColorConfig(symmetric_pattern=1))).elapsed_ms))
        order_ms = median_of(lambda: wall_ms(lambda: spmv.color_ordering(n, d_colors, colour.num_colors, d_perm,
                                                                         d_inverse)[0]))
        B = spmv.csr_create(0, 0, 0)
        permute_ms = median_of(lambda: wall_ms(lambda: spmv.csr_permute_gpu(B, A, d_perm, d_inverse)))
        src, dst = torch.empty(2 * nnz, dtype=torch.int32, device="cuda"), torch.empty(2 * nnz, dtype=torch.int32,
                                                                                      device="cuda")

        def copy_ms():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            dst.copy_(src)
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop)
        entry["reorder"] = {
            "colors": colour.num_colors, "rounds": colour.rounds, "launches": colour.launches,
            "rounds_seen": sorted({r.rounds for r in colour_runs}),
            "csr_color_ms": round(statistics.median(float(r.elapsed_ms) for r in colour_runs), 4),
            "csr_color_symmetric_pattern_ms": round(promised_ms, 4),
            "symmetric_pattern_same_colors": int(promised.num_colors == colour.num_colors),
            "color_ordering_wall_ms": round(order_ms, 4), "csr_permute_gpu_wall_ms": round(permute_ms, 4),
            "d2d_copy_of_the_entries_ms": round(median_of(copy_ms), 4), "entry_bytes_each_way": 8 * nnz}
        del src, dst

        note("reordered:", entry["reorder"])
        entry["natural"] = ordering_figures(A, n, nnz, d_b, d_x)
        note("natural ordering done")
        if spmv.permute_gather(d_pb, d_b, d_perm, n) != 0:
            raise RuntimeError("permute_gather failed")
        entry["coloured"] = ordering_figures(B, n, nnz, d_pb, d_x)
        steps = entry["coloured"]["cg_ic"]["iterations"]
        entry["coloured"]["launches_per_step_bound"] = 4 + 2 * colour.num_colors
        entry["natural"]["launches_per_step_bound"] = 4 + entry["natural"]["sptrsv_lower"]["launches"] + \
            entry["natural"]["sptrsv_upper"]["launches"]
        entry["time_to_solution_ms"] = {"ic_natural": entry["natural"]["cg_ic"]["ms_to_solution"],
                                        "ic_coloured": entry["coloured"]["cg_ic"]["ms_to_solution"],
                                        "jacobi": entry["natural"]["cg_jacobi"]["ms_to_solution"]}
        entry["coloured_steps_over_jacobi_steps"] = round(steps / max(entry["natural"]["cg_jacobi"]["iterations"], 1), 4)
        for buf in (d_b, d_pb, d_x, d_colors, d_perm, d_inverse):
            buf.release()
        spmv.csr_destroy(B)
        spmv.csr_destroy(A)
        result["matrices"][name.strip()] = entry
        print(name, json.dumps(entry), flush=True)

    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
