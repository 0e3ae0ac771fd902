"""bsr_ic_bench.py — block IC(0) on BSR (bsr_ic0 + cg_solve_bsr_ic) against the two yardsticks it has to be judged by, in
one process and one session on one device: ic0_csr + cg_solve_ic (engine 0) on the SAME matrix expanded to CSR, and
cg_solve_bsr with BLOCK_JACOBI.  The yardsticks are existing code, never the new code.

Matrices: the four SPD block structures of tools/cg_bsr_bench.py (s27_b3, s9_b2, s7_b4, poor_b4; about 10^6 scalar rows,
strictly diagonally dominant) and lap_k_b3, the weakly dominant (2-D 5-point Laplacian on a 578 x 578 grid) (x) K + 0.05 I
with K[i][j] = min(i, j) + 1, 1 002 252 scalar rows.

Per matrix and solver, medians and min - max over --runs after --warmup:
* the factorisation's device time, the levels of the schedule and the launches of one preconditioner apply;
* elapsed_ms / iterations at a fixed max_iterations (tolerance 0);
* iterations to 1e-6 and the device time of that solve; time to solution = factor + solve.

    python tools/bsr_ic_bench.py [--runs 5] [--warmup 2] [--steps 30] [--cases s27_b3,...] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bsr_bench import CASES, stencil_blocks  # noqa: E402
from cg_bsr_bench import spd_blocks  # noqa: E402

BLOCK_JACOBI = 2
ALL_CASES = tuple(CASES) + ("lap_k_b3",)


def laplacian_k(m, b):
    """(nodes, brp, bcols, values [blocks, b, b]) of (5-point Laplacian on m x m) (x) K + 0.05 I"""
    nodes, brp, bcols = stencil_blocks((m, m), "cross")
    block_row = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(brp))
    degree = (np.diff(brp) - 1).astype(np.float64)
    i = np.arange(b)
    K = (np.minimum(i[:, None], i[None, :]) + 1).astype(np.float64)
    on = block_row == bcols
    scale = np.where(on, degree[block_row], -1.0)
    values = scale[:, None, None] * K[None] + np.where(on, 0.05, 0.0)[:, None, None] * np.eye(b)[None]
    return nodes, brp, bcols, values.astype(np.float32)


def addr(p):
    return ctypes.cast(p, ctypes.c_void_p).value


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--cases", default=",".join(ALL_CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsr_ic_bench.json"))
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    os.environ.pop("SPMV_DEBUG", None)

    report = {"device": spmv.device_name(), "version": spmv.version(), "runs": args.runs, "warmup": args.warmup,
              "steps": args.steps, "cases": {}}
    stat = lambda t: [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]
    for name in args.cases.split(","):
        if name == "lap_k_b3":
            b = 3
            nodes, brp, bcols, values = laplacian_k(578, b)
        else:
            case = CASES[name]
            b = case["b"]
            nodes, brp, bcols = stencil_blocks(case["dims"], case["reach"])
            values = spd_blocks(nodes, brp, bcols, b, case["drop"])
        n = nodes * b
        B = spmv.bsr_from_arrays(n, n, b, brp, bcols, values)
        assert spmv.bsr_to_gpu(B) == 0
        A = spmv.csr_create(0, 0, 0)
        assert spmv.bsr_to_csr_gpu(A, B, 0) == 0              # the CSR expansion: the stored non-zeros
        nnz, blocks = A.contents.nnz, int(bcols.size)
        del values

        rhs = np.random.default_rng(sum(name.encode())).uniform(-1.0, 1.0, n).astype(np.float32)
        d_b, d_x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        d_f, d_l = spmv.CudaBuffer(blocks * b * b), spmv.CudaBuffer(nnz)
        d_b.copyFromHost(rhs, n)
        zero = np.zeros(n, np.float32)
        c, a = B.contents, A.contents
        F = spmv.bsr_wrap_device(n, n, b, blocks, addr(c.d_block_row_ptrs), addr(c.d_block_cols), d_f.get())
        L = spmv.csr_wrap_device(n, n, nnz, addr(a.d_row_ptrs), addr(a.d_col_indices), d_l.get())

        def factor_times(call):
            times, last = [], None
            for i in range(args.warmup + args.runs):
                last = call()
                assert last.error_code == 0, spmv.spmv_error_string(last.error_code)
                if i >= args.warmup:
                    times.append(last.elapsed_ms)
            return stat(times), last

        def per_step(solve):
            times = []
            for i in range(args.warmup + args.runs):
                d_x.copyFromHost(zero, n)
                res = solve(spmv.CGConfig(tolerance=0.0, max_iterations=args.steps, engine=0, preconditioner=BLOCK_JACOBI))
                if res.error_code != 0 or res.iterations != args.steps:
                    raise RuntimeError((spmv.spmv_error_string(res.error_code), res.iterations, res.breakdown))
                if i >= args.warmup:
                    times.append(res.elapsed_ms / res.iterations)
            return stat(times)

        def to_tolerance(solve):
            times, its = [], None
            for i in range(args.warmup + args.runs):
                d_x.copyFromHost(zero, n)
                res = solve(spmv.CGConfig(tolerance=1e-6, max_iterations=5000, engine=0, preconditioner=BLOCK_JACOBI))
                assert res.error_code == 0, spmv.spmv_error_string(res.error_code)
                its = res.iterations if res.converged else None
                if i >= args.warmup:
                    times.append(res.elapsed_ms)
            return its, stat(times)

        bsr_factor, fr = factor_times(lambda: spmv.bsr_ic0(B, d_f))
        csr_factor, cr = factor_times(lambda: spmv.ic0_csr(A, d_l))
        up_b = spmv.sptrsv_analyze_bsr(B, 1)
        up_c = spmv.sptrsv_analyze(A, 1)
        solvers = {
            "cg_solve_bsr_ic": lambda cfg: spmv.cg_solve_bsr_ic(B, F, d_b, d_x, cfg),
            "cg_solve_ic_csr": lambda cfg: spmv.cg_solve_ic(A, L, d_b, d_x, cfg),
            "cg_solve_bsr_block_jacobi": lambda cfg: spmv.cg_solve_bsr(B, d_b, d_x, cfg),
        }
        entry = {"scalar_rows": n, "block_dim": b, "nnz": int(nnz), "blocks": blocks,
                 "bsr_ic0": {"factor_ms": bsr_factor, "levels": fr.num_levels, "launches": fr.launches,
                             "lanes": fr.lanes_per_row, "bad_pivot": fr.bad_pivot,
                             "apply_launches": fr.launches + up_b.launches},
                 "ic0_csr": {"factor_ms": csr_factor, "levels": cr.num_levels, "launches": cr.launches,
                             "lanes": cr.lanes_per_row, "bad_pivot": cr.bad_pivot,
                             "apply_launches": cr.launches + up_c.launches}}
        for key, solve in solvers.items():
            its, solve_ms = to_tolerance(solve)
            factor = bsr_factor[0] if key == "cg_solve_bsr_ic" else csr_factor[0] if key == "cg_solve_ic_csr" else 0.0
            entry[key] = {"step_ms": per_step(solve), "iterations_to_1e-6": its, "solve_ms": solve_ms,
                          "time_to_solution_ms": round(factor + solve_ms[0], 4)}
        print(name, json.dumps(entry), flush=True)
        report["cases"][name] = entry
        for buf in (d_b, d_x, d_f, d_l):
            buf.release()
        spmv.bsr_destroy(F)
        spmv.csr_destroy(L)
        spmv.csr_destroy(A)
        spmv.bsr_destroy(B)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
