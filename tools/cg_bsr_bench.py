"""cg_bsr_bench.py — a step of cg_solve_bsr against the yardstick it has to beat, a step of cg_solve (engine 0, JACOBI)
on the SAME matrix expanded to CSR, in one process and one session.

Matrices: the four block structures of tools/bsr_bench.py (s27_b3, s9_b2, s7_b4, poor_b4; about 10^6 scalar rows)
made SPD.  Every off-diagonal scalar position (i, j) holds -u(i, j), u a symmetric hash in (0, 1); inside a diagonal
block the coupling is three times as strong; the scalar diagonal is the row's absolute sum plus one: symmetric and
strictly diagonally dominant.  poor_b4 drops a symmetric 45 % of the positions outside the diagonal blocks from the
CSR matrix; the BSR matrix stores them as padding.

Per matrix, medians and min - max over --runs solves after --warmup:
* elapsed_ms / iterations at a fixed max_iterations (tolerance 0) for cg_solve JACOBI on the CSR expansion and for
  cg_solve_bsr with JACOBI and with BLOCK_JACOBI, the ratio yardstick / BSR beside the byte model of a step;
* iterations to 1e-6 for JACOBI against BLOCK_JACOBI (one solve each);
* bsr_diag_inverse_gpu (wall time of the call, which ends in its read-back) in units of one cg_solve_bsr step.

    python tools/cg_bsr_bench.py [--runs 10] [--warmup 2] [--steps 50] [--cases s27_b3,...] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bsr_bench import CASES, stencil_blocks  # noqa: E402

NONE, JACOBI, BLOCK_JACOBI = 0, 1, 2


def symmetric_hash(i, j, salt):
    """u(i, j) = u(j, i) in (0, 1) for int64 index arrays"""
    lo, hi = np.minimum(i, j).astype(np.uint64), np.maximum(i, j).astype(np.uint64)
    h = (lo * np.uint64(2654435761) + hi * np.uint64(40503) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    h = (h * np.uint64(2246822519) + np.uint64(3266489917)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(668265263)) & np.uint64(0xFFFFFFFF)
    return (h.astype(np.float64) + 0.5) / 4294967296.0


def spd_blocks(nodes, brp, bcols, b, drop):
    """[blocks, b, b] float32 values of the SPD matrix over the block structure (module docstring)"""
    block_row = np.repeat(np.arange(nodes, dtype=np.int64), np.diff(brp))
    r = np.arange(b, dtype=np.int64)
    gi = (block_row[:, None, None] * b + r[None, :, None]) + np.zeros((1, 1, b), np.int64)
    gj = (bcols.astype(np.int64)[:, None, None] * b + r[None, None, :]) + np.zeros((1, b, 1), np.int64)
    values = -symmetric_hash(gi, gj, 1)
    inside = (block_row == bcols)[:, None, None]
    values = np.where(inside, 3.0 * values, values)
    if drop > 0:
        values = np.where(~inside & (symmetric_hash(gi, gj, 2) < drop), 0.0, values)
    values[gi == gj] = 0.0
    row_sum = np.bincount(gi.ravel(), weights=np.abs(values).ravel(), minlength=nodes * b)
    on = gi == gj
    values[on] = row_sum[gi[on]] + 1.0
    return values.astype(np.float32)


def step_bytes(n, nnz, blocks, block_rows, b):
    """Bytes a step must move at least: the matrix once; per row p, q of the product (2 floats), the update's reads of
    p, q, x, r and its factor and its writes of x, r (and z), and the direction step's reads and write."""
    csr = nnz * 8 + (n + 1) * 4 + n * 4 * (2 + 7 + 4)                 # dinv read twice, z never stored
    bsr_matrix = blocks * (4 * b * b + 4) + (block_rows + 1) * 4
    bsr_jacobi = bsr_matrix + n * 4 * (2 + 8 + 3)
    bsr_block = bsr_matrix + n * 4 * (2 + 7 + b + 3)
    return csr, bsr_jacobi, bsr_block


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cg_bsr_bench.json"))
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    os.environ.pop("SPMV_DEBUG", None)

    report = {"device": spmv.device_name(), "version": spmv.version(), "runs": args.runs, "warmup": args.warmup,
              "steps": args.steps, "cases": {}}
    for name in args.cases.split(","):
        case = CASES[name]
        b = case["b"]
        nodes, brp, bcols = stencil_blocks(case["dims"], case["reach"])
        n = nodes * b
        values = spd_blocks(nodes, brp, bcols, b, case["drop"])
        B = spmv.bsr_from_arrays(n, n, b, brp, bcols, values)
        assert spmv.bsr_to_gpu(B) == 0
        A = spmv.csr_create(0, 0, 0)
        assert spmv.bsr_to_csr_gpu(A, B, 0) == 0              # the CSR expansion: the stored non-zeros
        nnz, blocks = A.contents.nnz, int(bcols.size)
        del values

        rhs = np.random.default_rng(sum(name.encode())).uniform(-1.0, 1.0, n).astype(np.float32)
        d_b, d_x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        d_inv = spmv.CudaBuffer(nodes * b * b)
        d_b.copyFromHost(rhs, n)
        zero = np.zeros(n, np.float32)

        def per_step(solve):
            """(median, min, max) of elapsed_ms / iterations over the runs after the warm-ups"""
            times = []
            for i in range(args.warmup + args.runs):
                d_x.copyFromHost(zero, n)
                res = solve(spmv.CGConfig(tolerance=0.0, max_iterations=args.steps, engine=0))
                if res.error_code != 0 or res.iterations != args.steps:
                    raise RuntimeError((spmv.spmv_error_string(res.error_code), res.iterations))
                if i >= args.warmup:
                    times.append(res.elapsed_ms / res.iterations)
            return statistics.median(times), min(times), max(times)

        def with_precond(entry, M, precond):
            def solve(cfg):
                cfg.preconditioner = precond
                return entry(M, d_b, d_x, cfg)
            return solve

        def to_tolerance(entry, M, precond):
            d_x.copyFromHost(zero, n)
            res = entry(M, d_b, d_x, spmv.CGConfig(tolerance=1e-6, max_iterations=5000, engine=0, preconditioner=precond))
            assert res.error_code == 0, spmv.spmv_error_string(res.error_code)
            return res.iterations if res.converged else None

        csr = per_step(with_precond(spmv.cg_solve, A, JACOBI))
        bsr_j = per_step(with_precond(spmv.cg_solve_bsr, B, JACOBI))
        bsr_b = per_step(with_precond(spmv.cg_solve_bsr, B, BLOCK_JACOBI))
        bsr_n = per_step(with_precond(spmv.cg_solve_bsr, B, NONE))
        walls = []
        for i in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            assert spmv.bsr_diag_inverse_gpu(B, d_inv) == 0
            if i >= args.warmup:
                walls.append((time.perf_counter() - t0) * 1e3)
        model = step_bytes(n, nnz, blocks, nodes, b)
        r4 = lambda t: [round(v, 4) for v in t]
        entry = {
            "scalar_rows": n, "block_dim": b, "nnz": int(nnz), "blocks": blocks,
            "cg_solve_jacobi_step_ms": r4(csr), "cg_solve_bsr_jacobi_step_ms": r4(bsr_j),
            "cg_solve_bsr_block_jacobi_step_ms": r4(bsr_b), "cg_solve_bsr_none_step_ms": r4(bsr_n),
            "yardstick_spread_ms": round(csr[2] - csr[1], 4),
            "jacobi_step_gain_ms": round(csr[0] - bsr_j[0], 4),
            "speedup_bsr_jacobi_over_csr": round(csr[0] / bsr_j[0], 3),
            "speedup_bsr_block_jacobi_over_csr": round(csr[0] / bsr_b[0], 3),
            "step_bytes_csr": model[0], "step_bytes_bsr_jacobi": model[1], "step_bytes_bsr_block_jacobi": model[2],
            "byte_ratio_csr_over_bsr_jacobi": round(model[0] / model[1], 3),
            "csr_step_model_gb_s": round(model[0] / 1e6 / csr[0], 1),
            "bsr_jacobi_step_model_gb_s": round(model[1] / 1e6 / bsr_j[0], 1),
            "bsr_block_jacobi_step_model_gb_s": round(model[2] / 1e6 / bsr_b[0], 1),
            "iterations_to_1e-6": {"cg_solve_jacobi": to_tolerance(spmv.cg_solve, A, JACOBI),
                                   "cg_solve_bsr_jacobi": to_tolerance(spmv.cg_solve_bsr, B, JACOBI),
                                   "cg_solve_bsr_block_jacobi": to_tolerance(spmv.cg_solve_bsr, B, BLOCK_JACOBI)},
            "inverse_wall_ms": round(statistics.median(walls), 4),
            "inverse_in_bsr_block_jacobi_steps": round(statistics.median(walls) / bsr_b[0], 2),
        }
        print(name, json.dumps(entry), flush=True)
        report["cases"][name] = entry
        for buf in (d_b, d_x, d_inv):
            buf.release()
        spmv.csr_destroy(A)
        spmv.bsr_destroy(B)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
