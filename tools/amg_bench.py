"""amg_bench.py — time to solution of cg_solve_amg against Jacobi-preconditioned cg_solve, and the cost of amg_setup
and of amg_setup_device side by side.

Matrices (numpy, gpu-spmv_amd/spd.py): P2D1024, the 5-point 2-D Poisson matrix at 1024^2 (1.05 M rows), and P3D128,
the 7-point 3-D Poisson matrix at 128^3 (2.1 M rows).  Per matrix: amg_setup (--runs times after --warmup, a fresh
hierarchy each time; AMGResult.setup_ms and the wall time of the call), the same for amg_setup_device (seed 0) in the
same process, with the rounds its root selection took per level; then cg_solve with JACOBI and cg_solve_amg on each of
the two hierarchies from x0 = 0 to tolerance 1e-6 with the default engine (-1): --runs solves after --warmup, the wall
time of the call (setup of the solve, its read-backs and the loop) and the device-event time of the loop, each as the
median, and the iterations.  Nothing is presumed about the winner: `faster` names whichever solve has the smaller
median wall time, with and without one setup added to the AMG side; `device_over_host_setup` is the ratio of the two
setups' median wall times.

With --smoothed the same is measured, in the same process, for amg_setup_smoothed and amg_setup_smoothed_device
(default AMGSmoothing) and for cg_solve_amg on their hierarchies, and every smoothed row is compared with the plain row
of this very run: `smoothed_over_plain_*` are ratios of median wall times (below 1: smoothed is faster), with nothing
and with one setup added to both sides.

    python tools/amg_bench.py [--matrices P2D1024,P3D128] [--runs 10] [--warmup 2] [--out profiles/amg_bench.json]
    python tools/amg_bench.py --smoothed --out profiles/amg_smoothed_bench.json
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
    ap.add_argument("--matrices", default="P2D1024,P3D128")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--smoothed", action="store_true", help="add the smoothed-aggregation rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_bench.json"))
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    makers = {"P2D1024": lambda: spd.poisson2d(1024), "P3D128": lambda: spd.poisson3d(128),
              "P2D256": lambda: spd.poisson2d(256)}
    result = {"tool": "tools/amg_bench.py", "device": spmv.device_name(), "runs": args.runs, "warmup": args.warmup,
              "tolerance": args.tolerance, "statistic": "median over runs after the warm-up runs", "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        b, x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        b.copyFromHost(np.random.default_rng(7).uniform(-1.0, 1.0, n).astype(np.float32), n)
        zeros = np.zeros(n, np.float32)

        def time_setup(build):
            """(the entry, the last hierarchy): --runs builds after --warmup, a fresh hierarchy each time"""
            setup_ms, setup_wall, H, info = [], [], None, None
            for run in range(args.warmup + args.runs):
                spmv.amg_destroy(H)
                spmv.device_synchronize()
                t0 = time.perf_counter()
                info, H = build()
                wall = (time.perf_counter() - t0) * 1e3
                if info.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(info.error_code))
                if run >= args.warmup:
                    setup_ms.append(info.setup_ms)
                    setup_wall.append(wall)
            sizes = [spmv.amg_level(H, l)[1].num_rows for l in range(info.levels)]
            entries = [spmv.amg_level(H, l)[1].nnz for l in range(info.levels)]
            return {"setup_ms": round(statistics.median(setup_ms), 3),
                    "wall_ms": round(statistics.median(setup_wall), 3),
                    "wall_ms_min_max": [round(min(setup_wall), 3), round(max(setup_wall), 3)], "levels": info.levels,
                    "level_rows": sizes, "level_nnz": entries, "coarse_solver": info.coarse_solver,
                    "grid_complexity": round(info.grid_complexity, 4),
                    "operator_complexity": round(info.operator_complexity, 4)}, H

        entry = {"rows": n, "nnz": int(ci.size)}
        entry["amg_setup"], H = time_setup(lambda: spmv.amg_setup(A))
        entry["amg_setup_device"], HD = time_setup(lambda: spmv.amg_setup_device(A, None, 0))
        entry["amg_setup_device"]["rounds"] = [spmv.amg_setup_rounds(HD, l)
                                               for l in range(entry["amg_setup_device"]["levels"])]
        entry["device_over_host_setup"] = round(entry["amg_setup_device"]["wall_ms"] / entry["amg_setup"]["wall_ms"], 3)

        cfg = spmv.CGConfig(tolerance=args.tolerance, max_iterations=100000, preconditioner=1, engine=-1)
        solvers = {"cg_solve_jacobi": lambda: spmv.cg_solve(A, b, x, cfg),
                   "cg_solve_amg": lambda: spmv.cg_solve_amg(A, H, b, x, cfg),
                   "cg_solve_amg_device_setup": lambda: spmv.cg_solve_amg(A, HD, b, x, cfg)}
        if args.smoothed:
            entry["amg_setup_smoothed"], HS = time_setup(lambda: spmv.amg_setup_smoothed(A))
            entry["amg_setup_smoothed_device"], HSD = time_setup(lambda: spmv.amg_setup_smoothed_device(A, None, None, 0))
            entry["amg_setup_smoothed_device"]["rounds"] = [
                spmv.amg_setup_rounds(HSD, l) for l in range(entry["amg_setup_smoothed_device"]["levels"])]
            solvers["cg_solve_amg_smoothed"] = lambda: spmv.cg_solve_amg(A, HS, b, x, cfg)
            solvers["cg_solve_amg_smoothed_device_setup"] = lambda: spmv.cg_solve_amg(A, HSD, b, x, cfg)
        for label, solve in solvers.items():
            wall, loop, res = [], [], None
            for run in range(args.warmup + args.runs):
                x.copyFromHost(zeros, n)
                spmv.device_synchronize()
                t0 = time.perf_counter()
                res = solve()
                elapsed = (time.perf_counter() - t0) * 1e3
                if res.error_code != 0:
                    raise RuntimeError(label + ": " + spmv.spmv_error_string(res.error_code))
                if run >= args.warmup:
                    wall.append(elapsed)
                    loop.append(res.elapsed_ms)
            entry[label] = {"wall_ms": round(statistics.median(wall), 3), "loop_ms": round(statistics.median(loop), 3),
                            "iterations": res.iterations, "converged": res.converged, "breakdown": res.breakdown,
                            "relative_residual": res.relative_residual,
                            "ms_per_iteration": round(statistics.median(loop) / max(res.iterations, 1), 5)}
        jacobi, amg = entry["cg_solve_jacobi"]["wall_ms"], entry["cg_solve_amg"]["wall_ms"]
        entry["faster"] = "cg_solve_amg" if amg < jacobi else "cg_solve_jacobi"
        with_setup = amg + entry["amg_setup"]["wall_ms"]
        entry["faster_with_one_setup"] = "cg_solve_amg" if with_setup < jacobi else "cg_solve_jacobi"
        entry["jacobi_over_amg_wall"] = round(jacobi / amg, 3)
        amg_device = entry["cg_solve_amg_device_setup"]["wall_ms"]
        with_device_setup = amg_device + entry["amg_setup_device"]["wall_ms"]
        entry["faster_with_one_device_setup"] = "cg_solve_amg" if with_device_setup < jacobi else "cg_solve_jacobi"
        if args.smoothed:
            for solve, setup, plain_solve, plain_setup in (
                    ("cg_solve_amg_smoothed", "amg_setup_smoothed", "cg_solve_amg", "amg_setup"),
                    ("cg_solve_amg_smoothed_device_setup", "amg_setup_smoothed_device", "cg_solve_amg_device_setup",
                     "amg_setup_device")):
                smoothed, plain = entry[solve]["wall_ms"], entry[plain_solve]["wall_ms"]
                entry["smoothed_over_plain_" + solve] = {
                    "per_solve": round(smoothed / plain, 3),
                    "with_one_setup": round((smoothed + entry[setup]["wall_ms"]) / (plain + entry[plain_setup]["wall_ms"]), 3),
                    "setup": round(entry[setup]["wall_ms"] / entry[plain_setup]["wall_ms"], 3),
                    "ms_per_iteration": round(entry[solve]["ms_per_iteration"] / entry[plain_solve]["ms_per_iteration"], 3)}
            spmv.amg_destroy(HS)
            spmv.amg_destroy(HSD)
        result["matrices"][name] = entry
        spmv.amg_destroy(H)
        spmv.amg_destroy(HD)
        for buf in (b, x):
            buf.release()
        spmv.csr_destroy(A)

    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
