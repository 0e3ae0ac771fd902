"""ppr_bench.py — one pagerank_personalized step for k teleport vectors against k pagerank() steps.

Graphs (built in HBM, gpu-spmv_amd/workloads.py, made column-stochastic): C2 = uniform 1 M nodes x 16 links per row,
C4 = the 1 M-node power-law graph.  damping 0.85, tolerance 0, max_iterations 20, so every call runs exactly 20 steps;
k in {1, 4, 8, 16, 32} one-hot teleport vectors.

Batched side: the call's own elapsed_ms (device events around the loop of 20 steps), median of --runs calls after
--warmup; ms per step = that / 20.

Baseline: pagerank() as the library has it, same matrix, same 20 steps, in the same session but in a child process of
its own per engine (SPMV_TILED is read once per process): once with SPMV_TILED=0 (direct kernels) and once at its
default (the tiled engine; the warm-up calls build and cache the plan, so the timed calls run all 20 steps on it).
pagerank() reports no device time, so a step is the difference of two wall-clock medians: (a 20-step call - a 0-step
call) / 20, which removes the workspace, mask and copy-out work both calls share.

The one gate (reported, not enforced): on C2 at k = 32 a batched step costs at most half of 32 direct pagerank() steps.

    python tools/ppr_bench.py [--matrices C2,C4] [--ks 1,4,8,16,32] [--runs 10] [--warmup 2]
                              [--out profiles/ppr_bench.json]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1_000_000
STEPS = 20
DAMPING = 0.85


def build(spmv, name):
    wl = importlib.import_module("gpu-spmv_amd.workloads")
    A = wl.uniform_csr_device(42, N, N, 16) if name == "C2" else wl.power_law_csr_device(42, N, N)
    wl.make_column_stochastic(A).release()
    return A


def baseline(args) -> int:
    """Child process: pagerank() on one matrix with whatever engine the environment selects."""
    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    A = build(spmv, args.baseline)
    walls = {STEPS: [], 0: []}
    iterations = None
    for rep in range(args.warmup + args.runs):
        for steps in (STEPS, 0):
            t0 = time.perf_counter()
            r = spmv.pagerank(A.handle, spmv.PageRankConfig(DAMPING, 0.0, steps))
            t = (time.perf_counter() - t0) * 1e3
            assert r.ranks is not None and r.iterations == steps, (r.iterations, steps)
            if steps:
                iterations = r.iterations
            del r
            if rep >= args.warmup:
                walls[steps].append(t)
    full, empty = statistics.median(walls[STEPS]), statistics.median(walls[0])
    print(json.dumps({"engine": "tiled" if spmv.csr_has_tiled_plan(A.handle) else "direct", "iterations": iterations,
                      "wall_ms_20_steps": round(full, 4), "wall_ms_0_steps": round(empty, 4),
                      "ms_per_step": round((full - empty) / STEPS, 5)}))
    A.close()
    return 0


def run_baseline(name, tiled, args):
    env = dict(os.environ)
    env.pop("SPMV_DEBUG", None)
    if tiled:
        env.pop("SPMV_TILED", None)
    else:
        env["SPMV_TILED"] = "0"
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline", name, "--runs", str(args.runs),
                          "--warmup", str(args.warmup)], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError("baseline %s failed:\n%s%s" % (name, out.stdout, out.stderr))
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["engine"] == ("tiled" if tiled else "direct"), got
    return got


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="C2,C4")
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppr_bench.json"))
    args = ap.parse_args()
    if args.baseline:
        return baseline(args)

    import numpy as np

    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    ks = [int(k) for k in args.ks.split(",")]
    cfg = spmv.PageRankConfig(DAMPING, 0.0, STEPS)
    result = {"tool": "tools/ppr_bench.py", "device": spmv.device_name(), "runs": args.runs, "warmup": args.warmup,
              "settings": "damping 0.85, tolerance 0, 20 steps, one-hot teleport vectors",
              "statistic": "batched: median elapsed_ms (device events) / 20; pagerank(): (median wall of a 20-step call "
                           "- median wall of a 0-step call) / 20, each engine in a process of its own",
              "matrices": {}}
    for name in args.matrices.split(","):
        direct = run_baseline(name, False, args)
        tiled = run_baseline(name, True, args)
        print(name, "pagerank() direct", json.dumps(direct), flush=True)
        print(name, "pagerank() tiled", json.dumps(tiled), flush=True)
        A = build(spmv, name)
        entry = {"rows": N, "nnz": A.nnz, "pagerank_direct": direct, "pagerank_tiled": tiled, "k": {}}
        for k in ks:
            V = np.zeros((N, k), np.float32)
            V[1000 * np.arange(k) + 17, np.arange(k)] = 1.0
            d_V, d_R = spmv.CudaBuffer(N * k), spmv.CudaBuffer(N * k)
            d_V.copyFromHost(V.ravel(), N * k)
            device_ms, wall_ms = [], []
            for rep in range(args.warmup + args.runs):
                t0 = time.perf_counter()
                results = spmv.pagerank_personalized(A.handle, d_V, d_R, k, config=cfg)
                t = (time.perf_counter() - t0) * 1e3
                if results[0].error_code != 0:
                    raise RuntimeError(spmv.spmv_error_string(results[0].error_code))
                assert all(r.iterations == STEPS for r in results)
                if rep >= args.warmup:
                    device_ms.append(results[0].elapsed_ms)
                    wall_ms.append(t)
            sums = d_R.copyToHost(N * k).reshape(N, k).sum(axis=0, dtype=np.float64)
            d_V.release()
            d_R.release()
            step = statistics.median(device_ms) / STEPS
            entry["k"][str(k)] = {
                "ms_per_step": round(step, 5), "ms_per_step_per_column": round(step / k, 5),
                "wall_ms_per_call": round(statistics.median(wall_ms), 3),
                "over_k_direct_steps": round(step / (k * direct["ms_per_step"]), 4),
                "over_k_tiled_steps": round(step / (k * tiled["ms_per_step"]), 4),
                "column_sums_within_1e-5_of_1": bool(np.all(np.abs(sums - 1.0) < 1e-5))}
            print(name, k, json.dumps(entry["k"][str(k)]), flush=True)
        if name == "C2" and "32" in entry["k"]:
            entry["gate_k32_at_most_half_of_32_direct_steps"] = bool(entry["k"]["32"]["over_k_direct_steps"] <= 0.5)
        A.close()
        result["matrices"][name] = entry

    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
