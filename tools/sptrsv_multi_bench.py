"""sptrsv_multi_bench.py — the k-wide triangular solve and IC-preconditioned batched CG against their single-column
calls.

Matrices (numpy, gpu-spmv_amd/spd.py): P2D = poisson2d(1024) (1.0 M rows, 2047 levels of at most 1024 rows, 1537
launches per solve), P3D = poisson3d(128) (2.1 M rows, 382 levels, 340 launches per solve).  F = ic0_csr(A) wrapped over
A's structure.  k in {1, 2, 4, 8, 16, 32} uniform random columns (column j is the same whatever k).  Everything runs in
this one process on one build; the analysis and both schedules are built before anything is timed; --runs timed
repetitions after --warmup untimed ones; wall time around the calls alone (uploads are not timed; each call returns
after its work).  A repetition of a single side runs all 32 columns one after the other and times each, so the sum for
k is the time of the first k calls of that repetition; medians are over repetitions.

Sections:
  sptrsv   sptrsv_csr_multi on F (LOWER and UPPER, NON_UNIT, ordered = 0) against k sptrsv_csr calls.
  cg_steps cg_solve_multi_ic against k cg_solve_ic(engine = 0) calls, both stopped after --cg-steps steps (tolerance 0):
           the cost of a step, where a full solve of P2D is too long to repeat 12 x 32 times.
  cg_full  cg_solve_multi_ic against cg_solve_multi with JACOBI, both to tolerance 1e-6 (--full-matrices).
Every batched column is checked against its single call (the bits of x, and the iterations where there are any); the
result says so per row.

    python tools/sptrsv_multi_bench.py [--matrices P2D,P3D] [--full-matrices P3D] [--ks 1,2,4,8,16,32] [--runs 10]
                                       [--warmup 2] [--cg-steps 5] [--out profiles/sptrsv_multi_bench.json]
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
    ap.add_argument("--full-matrices", default="P3D")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cg-steps", type=int, default=5)
    ap.add_argument("--max-iterations", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sptrsv_multi_bench.json"))
    args = ap.parse_args()

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    ks = [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    reps = args.warmup + args.runs
    makers = {"P2D": lambda: spd.poisson2d(1024), "P3D": lambda: spd.poisson3d(128)}
    full = set(filter(None, args.full_matrices.split(",")))
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)

    def ok(code):
        if code != 0:
            raise RuntimeError(spmv.spmv_error_string(code))

    result = {"tool": "tools/sptrsv_multi_bench.py", "device": spmv.device_name(), "runs": args.runs,
              "warmup": args.warmup, "cg_steps": args.cg_steps,
              "statistic": "median wall ms over runs; single = the first k of 32 single-column calls of a repetition",
              "matrices": {}}

    for name in args.matrices.split(","):
        n, rp, ci, va = makers[name]()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        ok(spmv.csr_to_gpu(A))
        d_l = spmv.CudaBuffer(ci.size)
        ok(spmv.ic0_csr(A, d_l).error_code)
        F = spmv.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, d_l.get())
        shape = {u: spmv.sptrsv_analyze(F, u) for u in (0, 1)}        # both schedules, ahead of every timed call
        B = np.random.default_rng(7).uniform(-1.0, 1.0, (n, kmax)).astype(np.float32)
        entry = {"rows": n, "nnz": int(ci.size),
                 "levels": shape[0].num_levels, "launches_per_solve": [shape[0].launches, shape[1].launches],
                 "sptrsv": {}, "cg_steps": {}, "cg_full": {}}
        d_b = [spmv.CudaBuffer(n) for _ in range(kmax)]
        for j in range(kmax):
            d_b[j].copyFromHost(np.ascontiguousarray(B[:, j]), n)
        d_x = spmv.CudaBuffer(n)
        zeros = np.zeros(n, np.float32)

        # ---- sptrsv: the single side, both triangles, every column timed
        single_wall = {0: [], 1: []}
        single_x = {0: [None] * kmax, 1: [None] * kmax}
        lanes = {}
        for uplo in (0, 1):
            cfg = spmv.SpTRSVConfig(uplo=uplo)
            for rep in range(reps):
                wall = []
                for j in range(kmax):
                    t0 = time.perf_counter()
                    res = spmv.sptrsv_csr(F, d_b[j], d_x, cfg)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ok(res.error_code)
                    lanes[uplo] = res.lanes_per_row
                    if rep == 0:
                        single_x[uplo][j] = d_x.copyToHost(n)
                if rep >= args.warmup:
                    single_wall[uplo].append(wall)
        single_wall = {u: np.asarray(w) for u, w in single_wall.items()}
        entry["lanes_per_row"] = [lanes[0], lanes[1]]
        for k in ks:
            d_B, d_X = spmv.CudaBuffer(n * k), spmv.CudaBuffer(n * k)
            d_B.copyFromHost(np.ascontiguousarray(B[:, :k]).ravel(), n * k)
            row = {}
            for uplo, tag in ((0, "lower"), (1, "upper")):
                cfg = spmv.SpTRSVConfig(uplo=uplo)
                wall, res = [], None
                for rep in range(reps):
                    t0 = time.perf_counter()
                    res = spmv.sptrsv_csr_multi(F, d_B, d_X, k, config=cfg)
                    t = (time.perf_counter() - t0) * 1e3
                    ok(res.error_code)
                    if rep >= args.warmup:
                        wall.append(t)
                X = d_X.copyToHost(n * k).reshape(n, k)
                same = all(np.array_equal(bits(X[:, j]), bits(single_x[uplo][j])) for j in range(k))
                multi_ms = statistics.median(wall)
                single_ms = float(np.median(single_wall[uplo][:, :k].sum(axis=1)))
                row[tag] = {"multi_wall_ms": round(multi_ms, 3), "single_sum_wall_ms": round(single_ms, 3),
                            "single_over_multi": round(single_ms / multi_ms, 3), "launches": res.launches,
                            "multi_device_ms": round(res.elapsed_ms, 3), "columns_bit_equal_to_single": bool(same)}
            entry["sptrsv"][str(k)] = row
            print(name, "sptrsv", k, json.dumps(row), flush=True)
            d_B.release()
            d_X.release()

        # ---- cg, stopped after --cg-steps steps: k singles against one batched call
        capped = spmv.CGConfig(tolerance=0.0, max_iterations=args.cg_steps, engine=0)
        single_wall, single_x, single_it = [], [None] * kmax, [0] * kmax
        for rep in range(reps):
            wall = []
            for j in range(kmax):
                d_x.copyFromHost(zeros, n)
                t0 = time.perf_counter()
                res = spmv.cg_solve_ic(A, F, d_b[j], d_x, capped)
                wall.append((time.perf_counter() - t0) * 1e3)
                ok(res.error_code)
                single_it[j] = res.iterations
                if rep == 0:
                    single_x[j] = d_x.copyToHost(n)
            if rep >= args.warmup:
                single_wall.append(wall)
        single_wall = np.asarray(single_wall)
        for k in ks:
            d_B, d_X = spmv.CudaBuffer(n * k), spmv.CudaBuffer(n * k)
            d_B.copyFromHost(np.ascontiguousarray(B[:, :k]).ravel(), n * k)
            zeros_k = np.zeros(n * k, np.float32)
            wall, results = [], None
            for rep in range(reps):
                d_X.copyFromHost(zeros_k, n * k)
                t0 = time.perf_counter()
                results = spmv.cg_solve_multi_ic(A, F, d_B, d_X, k, config=capped)
                t = (time.perf_counter() - t0) * 1e3
                ok(results[0].error_code)
                if rep >= args.warmup:
                    wall.append(t)
            X = d_X.copyToHost(n * k).reshape(n, k)
            same = all(results[j].iterations == single_it[j] and np.array_equal(bits(X[:, j]), bits(single_x[j]))
                       for j in range(k))
            multi_ms = statistics.median(wall)
            single_ms = float(np.median(single_wall[:, :k].sum(axis=1)))
            row = {"steps": args.cg_steps, "multi_wall_ms": round(multi_ms, 3),
                   "single_sum_wall_ms": round(single_ms, 3), "single_over_multi": round(single_ms / multi_ms, 3),
                   "multi_loop_ms_per_step": round(results[0].elapsed_ms / max(args.cg_steps, 1), 4),
                   "columns_bit_equal_to_single": bool(same)}
            entry["cg_steps"][str(k)] = row
            print(name, "cg_steps", k, json.dumps(row), flush=True)

            # ---- to tolerance 1e-6: IC against JACOBI, both batched
            if name in full:
                row = {}
                for tag, call in (("ic", lambda cfg: spmv.cg_solve_multi_ic(A, F, d_B, d_X, k, config=cfg)),
                                  ("jacobi", lambda cfg: spmv.cg_solve_multi(A, d_B, d_X, k, config=cfg))):
                    cfg = spmv.CGConfig(tolerance=1e-6, max_iterations=args.max_iterations, preconditioner=1, engine=0)
                    wall, results = [], None
                    for rep in range(reps):
                        d_X.copyFromHost(zeros_k, n * k)
                        t0 = time.perf_counter()
                        results = call(cfg)
                        t = (time.perf_counter() - t0) * 1e3
                        ok(results[0].error_code)
                        if rep >= args.warmup:
                            wall.append(t)
                    row[tag] = {"wall_ms": round(statistics.median(wall), 3),
                                "steps": max(r.iterations for r in results),
                                "all_converged": all(bool(r.converged) for r in results)}
                row["jacobi_over_ic"] = round(row["jacobi"]["wall_ms"] / row["ic"]["wall_ms"], 3)
                entry["cg_full"][str(k)] = row
                print(name, "cg_full", k, json.dumps(row), flush=True)
            d_B.release()
            d_X.release()

        for buf in d_b + [d_x, d_l]:
            buf.release()
        spmv.csr_destroy(F)
        spmv.csr_destroy(A)
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
