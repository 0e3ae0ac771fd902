"""rcm_bench.py — what reverse Cuthill-McKee buys a matrix that arrives in an arbitrary numbering.

On symmetrically shuffled poisson2d(512) and poisson3d(160) (gpu-spmv_amd/spd.py), in one process:

* csr_rcm on the shuffled matrix: elapsed_ms, launches, sweeps, levels, components; the wall time of csr_permute_gpu;
* the band (csr_band_gpu) before and after;
* per ordering (natural = as generated, shuffled = P A P^T for a random P, rcm = the shuffled matrix reordered):
  spmv_csr VECTOR_CSR time and algorithmic GB/s (the byte model of spmv/bandwidth.h: 12 B per entry, 4 B per row
  pointer, x and y once), and cg_solve_ic to 1e-6: steps and milliseconds, with ic0_csr's time.

Every device time is the library's own elapsed_ms, the median of --runs after one warm-up.  Every GPU step runs under
a time limit of its own (--step-timeout seconds): when one runs out the tool writes what it has and ends with status 3
without starting another (the limit is an alarm, seen when the library call in flight returns; a call that never
returns is the caller's `timeout` to end).

    python tools/rcm_bench.py [--runs 3] [--matrices "poisson2d(512),poisson3d(160)"] [--out profiles/rcm_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import re
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL = 1e-6
VECTOR_CSR = 1


class StepTimeout(Exception):
    pass


def shuffled(n, rp, ci, va, seed):
    """P A P^T with sorted rows for the permutation default_rng(seed) draws (tests/rcm_cases.py shuffle, vectorised)"""
    p = np.random.default_rng(seed).permutation(n)
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    rows = inv[np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))]
    cols = inv[np.asarray(ci, np.int64)]
    order = np.lexsort((cols, rows))
    new_rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return n, new_rp, cols[order].astype(np.int32), np.asarray(va, np.float32)[order]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--matrices", default="poisson2d(512),poisson3d(160)")
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    spmv = importlib.import_module("gpu-spmv_amd")
    spd = importlib.import_module("gpu-spmv_amd.spd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)

    def note(*what):
        print("[rcm_bench]", *what, file=sys.stderr, flush=True)

    def on_alarm(signum, frame):
        raise StepTimeout()
    signal.signal(signal.SIGALRM, on_alarm)

    def step(name, call):
        """one GPU step under its own time limit"""
        signal.alarm(args.step_timeout)
        try:
            return call()
        except StepTimeout:
            note("step", name, "ran past", args.step_timeout, "s")
            raise
        finally:
            signal.alarm(0)

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

    def ordering_figures(label, M, n, nnz, b):
        out = {}
        status, lower, upper, profile = step(label + " band", lambda: spmv.csr_band_gpu(M))
        if status != 0:
            raise RuntimeError(spmv.spmv_error_string(status))
        out["band"] = {"lower": lower, "upper": upper, "profile": profile}
        d_b, d_x = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        d_b.copyFromHost(b, n)
        cfg = spmv.SpMVConfig(kernel_type=VECTOR_CSR)
        ms = step(label + " spmv", lambda: median_of(lambda: float(ok(spmv.spmv_csr(M, d_b, d_x, cfg, n)).elapsed_ms)))
        model_bytes = 12 * nnz + 4 * (n + 1) + 8 * n
        out["spmv_vector_csr"] = {"elapsed_ms": round(ms, 5), "algorithmic_gb_s": round(model_bytes / ms / 1e6, 1)}
        d_l = spmv.CudaBuffer(nnz)
        out["ic0_ms"] = round(step(label + " ic0", lambda: median_of(lambda: float(ok(spmv.ic0_csr(M, d_l)).elapsed_ms))), 4)
        F = spmv.csr_wrap_device(n, n, nnz, M.contents.d_row_ptrs, M.contents.d_col_indices, d_l.get())
        zeros = np.zeros(n, np.float32)

        def solve():
            d_x.copyFromHost(zeros, n)
            return ok(spmv.cg_solve_ic(M, F, d_b, d_x, spmv.CGConfig(tolerance=TOL)))

        def solves():
            solve()
            return [solve() for _ in range(args.runs)]
        runs = step(label + " cg_solve_ic", solves)
        ms = statistics.median(float(r.elapsed_ms) for r in runs)
        its = runs[-1].iterations
        out["cg_solve_ic"] = {"steps": its, "converged": int(runs[-1].converged), "ms": round(ms, 3),
                              "ms_per_step": round(ms / max(its, 1), 5)}
        for name, uplo in (("lower", 0), ("upper", 1)):
            out["sptrsv_levels_" + name] = ok(spmv.sptrsv_analyze(M, uplo)).num_levels
        spmv.csr_destroy(F)
        for buf in (d_b, d_x, d_l):
            buf.release()
        return out

    result = {"tool": "tools/rcm_bench.py", "device": spmv.device_name(), "runs": args.runs, "tolerance": TOL,
              "statistic": "median of runs after one warm-up; device times are the library's elapsed_ms, "
                           "csr_permute_gpu host wall time of the synchronous call",
              "complete": False, "matrices": {}}

    def write():
        print(json.dumps(result))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    try:
        for name in args.matrices.split(","):
            kind, size = re.fullmatch(r"(poisson[23]d)\((\d+)\)", name.strip()).groups()
            n, rp, ci, va = getattr(spd, kind)(int(size))
            nnz = int(ci.size)
            entry = {"rows": n, "nnz": nnz}
            result["matrices"][name.strip()] = entry
            b = np.random.default_rng(1).uniform(-1.0, 1.0, n).astype(np.float32)
            natural = spmv.csr_from_arrays(n, n, rp, ci, va)
            sn, srp, sci, sva = shuffled(n, rp, ci, va, 1)
            A = spmv.csr_from_arrays(n, n, srp, sci, sva)
            if spmv.csr_to_gpu(natural) != 0 or spmv.csr_to_gpu(A) != 0:
                raise RuntimeError("csr_to_gpu failed")
            note(name, "on the device:", n, "rows,", nnz, "entries")

            d_perm, d_inverse = spmv.CudaBuffer(n, "int32"), spmv.CudaBuffer(n, "int32")
            runs = step("csr_rcm", lambda: [ok(spmv.csr_rcm(A, d_perm, d_inverse)) for _ in range(args.runs + 1)][1:])
            promised = step("csr_rcm promised", lambda: [
                ok(spmv.csr_rcm(A, d_perm, d_inverse, spmv.RcmConfig(symmetric_pattern=1)))
                for _ in range(args.runs + 1)][1:])
            rcm = runs[-1]
            B = spmv.csr_create(0, 0, 0)
            permute_ms = step("csr_permute_gpu", lambda: median_of(
                lambda: wall_ms(lambda: spmv.csr_permute_gpu(B, A, d_perm, d_inverse))))
            wall = step("csr_rcm wall", lambda: median_of(lambda: wall_ms(
                lambda: spmv.csr_rcm(A, d_perm, d_inverse).error_code)))
            entry["csr_rcm"] = {
                "elapsed_ms": round(statistics.median(float(r.elapsed_ms) for r in runs), 3),
                "elapsed_ms_symmetric_pattern": round(statistics.median(float(r.elapsed_ms) for r in promised), 3),
                "wall_ms_with_the_builders": round(wall, 3),
                "launches": rcm.launches, "sweeps": rcm.sweeps, "levels": rcm.levels, "components": rcm.components,
                "csr_permute_gpu_wall_ms": round(permute_ms, 3)}
            note("reordered:", entry["csr_rcm"])
            entry["natural"] = ordering_figures("natural", natural, n, nnz, b)
            note("natural:", entry["natural"])
            entry["shuffled"] = ordering_figures("shuffled", A, n, nnz, b)
            note("shuffled:", entry["shuffled"])
            entry["rcm"] = ordering_figures("rcm", B, n, nnz, b)
            note("rcm:", entry["rcm"])
            entry["spmv_speedup_rcm_over_shuffled"] = round(
                entry["shuffled"]["spmv_vector_csr"]["elapsed_ms"] / entry["rcm"]["spmv_vector_csr"]["elapsed_ms"], 3)
            for buf in (d_perm, d_inverse):
                buf.release()
            for M in (natural, A, B):
                spmv.csr_destroy(M)
        result["complete"] = True
    except StepTimeout:
        write()
        return 3
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
