"""cg_multi_bench.py — one cg_solve_multi against k cg_solve(engine = 0) calls on the same columns.

Matrices (numpy, gpu-spmv_amd/spd.py): P2D = poisson2d(1024) (1.0 M rows, 5.2 M entries), P3D = poisson3d(128)
(2.1 M rows, 14.6 M entries).  JACOBI, tolerance 1e-6, x0 = 0, k in {1, 2, 4, 8, 16, 32} uniform random right-hand
sides (column j is the same whatever k).  Both sides run in this one process on the same build: --runs timed
repetitions after --warmup untimed ones, wall time around the calls alone (the uploads of B and x0 are not timed; each
call returns after its solve).  A repetition of the single side solves all 32 columns one after the other and times
each, so the sum for k is the time of the first k calls of that repetition; medians are over repetitions.
ms per step: the batched loop's elapsed_ms over the steps it ran (the slowest column's iterations); on the single
side the summed elapsed_ms over the summed iterations.  Every batched column is also checked against its single
solve (iterations and the bits of x) — the contract the tests hold, here at benchmark size.

    python tools/cg_multi_bench.py [--matrices P2D,P3D] [--ks 1,2,4,8,16,32] [--runs 10] [--warmup 2]
                                   [--out profiles/cg_multi_bench.json]
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
    ap.add_argument("--matrices", default="P2D,P3D")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_multi_bench.json"))
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    ks = [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    makers = {"P2D": lambda: spd.poisson2d(1024), "P3D": lambda: spd.poisson3d(128)}
    cfg = spmv.CGConfig(tolerance=1e-6, max_iterations=args.max_iterations, preconditioner=1, engine=0)
    result = {"tool": "tools/cg_multi_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "settings": "JACOBI, tolerance 1e-6, x0 = 0, engine 0, uniform random columns",
              "statistic": "median wall ms over runs; single = the first k of 32 cg_solve calls of a repetition",
              "matrices": {}}
    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        B = np.random.default_rng(7).uniform(-1.0, 1.0, (n, kmax)).astype(np.float32)
        entry = {"rows": n, "nnz": int(ci.size), "k": {}}

        # the single side: every column on its own, each call timed
        d_b = [spmv.CudaBuffer(n) for _ in range(kmax)]
        for j in range(kmax):
            d_b[j].copyFromHost(np.ascontiguousarray(B[:, j]), n)
        d_x = spmv.CudaBuffer(n)
        zeros = np.zeros(n, np.float32)
        single_wall, single_res, single_x = [], None, [None] * kmax
        for rep in range(args.warmup + args.runs):
            wall, res_list = [], []
            for j in range(kmax):
                d_x.copyFromHost(zeros, n)
                t0 = time.perf_counter()
                res = spmv.cg_solve(A, d_b[j], d_x, cfg)
                wall.append((time.perf_counter() - t0) * 1e3)
                if res.error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(res.error_code))
                res_list.append((res.iterations, res.converged, res.elapsed_ms))
                if rep == 0:
                    single_x[j] = d_x.copyToHost(n)
            if rep >= args.warmup:
                single_wall.append(wall)
            single_res = res_list
        for buf in d_b:
            buf.release()
        d_x.release()
        single_wall = np.asarray(single_wall)

        for k in ks:
            d_B, d_X = spmv.CudaBuffer(n * k), spmv.CudaBuffer(n * k)
            d_B.copyFromHost(np.ascontiguousarray(B[:, :k]).ravel(), n * k)
            zeros_k = np.zeros(n * k, np.float32)
            wall, results = [], None
            for rep in range(args.warmup + args.runs):
                d_X.copyFromHost(zeros_k, n * k)
                t0 = time.perf_counter()
                results = spmv.cg_solve_multi(A, d_B, d_X, k, config=cfg)
                t = (time.perf_counter() - t0) * 1e3
                if results[0].error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(results[0].error_code))
                if rep >= args.warmup:
                    wall.append(t)
            X = d_X.copyToHost(n * k).reshape(n, k)
            same = all(results[j].iterations == single_res[j][0] and
                       np.array_equal(X[:, j].view(np.uint32), single_x[j].view(np.uint32)) for j in range(k))
            d_B.release()
            d_X.release()
            steps = max(r.iterations for r in results)
            multi_ms = statistics.median(wall)
            single_ms = float(np.median(single_wall[:, :k].sum(axis=1)))
            single_iters = sum(single_res[j][0] for j in range(k))
            entry["k"][str(k)] = {
                "multi_wall_ms": round(multi_ms, 3), "single_sum_wall_ms": round(single_ms, 3),
                "single_over_multi": round(single_ms / multi_ms, 3),
                "steps": steps, "iterations": [r.iterations for r in results],
                "all_converged": all(r.converged for r in results) and all(single_res[j][1] for j in range(k)),
                "multi_ms_per_step": round(results[0].elapsed_ms / max(steps, 1), 5),
                "single_ms_per_step": round(sum(single_res[j][2] for j in range(k)) / max(single_iters, 1), 5),
                "columns_bit_equal_to_single": bool(same)}
            print(name, k, json.dumps(entry["k"][str(k)]), flush=True)
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
