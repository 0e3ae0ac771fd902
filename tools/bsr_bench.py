"""bsr_bench.py — spmv_bsr against the yardstick it has to beat, spmv_csr VECTOR_CSR (the direct kernel, use_texture =
false, promotion off) on the SAME matrix expanded to CSR, plus what the conversion costs.

Matrices (block structures built with numpy from a grid stencil, values uniform in [-1, 1], uploaded as BSR; the CSR
twin is bsr_to_csr_gpu of it, so both formats hold the same numbers):

* s27_b3   3-D 27-point stencil on 70^3 nodes, full 3x3 blocks   (1 029 000 scalar rows)
* s9_b2    2-D 9-point stencil on 720^2 nodes, full 2x2 blocks   (1 036 800 scalar rows)
* s7_b4    3-D 7-point stencil on 64^3 nodes, full 4x4 blocks    (1 048 576 scalar rows)
* poor_b4  s7_b4 with a random 45 % of every block's off-diagonal positions removed from the CSR matrix: fill near
           the break-even 1/2 + 1/(2 b^2) = 0.53 of the byte model; the BSR matrix stores them as padding

Per matrix: medians over --runs calls after --warmup of elapsed_ms (device events inside the call) of spmv_bsr
VECTOR_CSR, spmv_bsr SCALAR_CSR and spmv_csr VECTOR_CSR, their byte-model GB/s, the ratio csr / bsr beside the byte
ratio of the two models, the same for every forced lane count (SPMV_DEBUG=bsr_lanes=N), and bsr_from_csr_gpu
(symbolic_ms + numeric_ms and the wall time of the call) in units of one spmv_csr.  One process, one device, one
session: ratios between lines of one run are meaningful, absolute times move by several per cent from box to box.

    python tools/bsr_bench.py [--runs 10] [--warmup 2] [--cases s27_b3,s9_b2,s7_b4,poor_b4] [--out FILE]
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

CASES = {
    "s27_b3": dict(dims=(70, 70, 70), reach="box", b=3, drop=0.0),
    "s9_b2": dict(dims=(720, 720), reach="box", b=2, drop=0.0),
    "s7_b4": dict(dims=(64, 64, 64), reach="cross", b=4, drop=0.0),
    "poor_b4": dict(dims=(64, 64, 64), reach="cross", b=4, drop=0.45),
}


def stencil_blocks(dims, reach):
    """(block_row_ptrs, block_cols) of the node graph: every node with its neighbours in the box (3^d - point) or
    the cross (2 d + 1 - point) stencil, block columns ascending."""
    grids = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    coords = [g.reshape(-1) for g in grids]
    nodes = coords[0].size
    offsets = np.array(np.meshgrid(*[[-1, 0, 1]] * len(dims), indexing="ij")).reshape(len(dims), -1).T
    if reach == "cross":
        offsets = offsets[np.abs(offsets).sum(axis=1) <= 1]
    rows, cols = [], []
    for off in offsets:                                      # lexicographic offsets: ascending neighbour index
        ok = np.ones(nodes, bool)
        other = np.zeros(nodes, np.int64)
        for axis, d in enumerate(dims):
            c = coords[axis] + off[axis]
            ok &= (c >= 0) & (c < d)
            other = other * d + c
        rows.append(np.flatnonzero(ok))
        cols.append(other[ok])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((cols, rows))
    brp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nodes))]).astype(np.int32)
    return nodes, brp, cols[order].astype(np.int32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsr_bench.json"))
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)                              # the yardstick is the direct VECTOR_CSR kernel
    os.environ.pop("SPMV_DEBUG", None)
    vector = spmv.SpMVConfig(kernel_type=spmv.SpMVConfig.VECTOR_CSR, use_texture=False)
    scalar = spmv.SpMVConfig(kernel_type=spmv.SpMVConfig.SCALAR_CSR)

    def timed(call):
        """(median, min, max) of elapsed_ms over the runs after the warm-ups."""
        times = []
        for i in range(args.warmup + args.runs):
            res = call()
            if res.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(res.error_code))
            if i >= args.warmup:
                times.append(res.elapsed_ms)
        return statistics.median(times), min(times), max(times)

    report = {"device": spmv.device_name(), "version": spmv.version(), "runs": args.runs, "warmup": args.warmup, "cases": {}}
    for name in args.cases.split(","):
        case = CASES[name]
        b = case["b"]
        rng = np.random.default_rng(sum(name.encode()))
        nodes, brp, bcols = stencil_blocks(case["dims"], case["reach"])
        n = nodes * b
        values = rng.uniform(-1.0, 1.0, size=(bcols.size, b, b)).astype(np.float32)
        values[values == 0] = 0.5
        if case["drop"] > 0:
            gone = rng.random(values.shape) < case["drop"]
            diagonal = np.repeat(np.arange(nodes), np.diff(brp)) == bcols
            gone[diagonal[:, None, None] & np.eye(b, dtype=bool)[None]] = False
            values[gone] = 0.0
        full = spmv.bsr_from_arrays(n, n, b, brp, bcols, values)
        assert spmv.bsr_to_gpu(full) == 0
        A = spmv.csr_create(0, 0, 0)
        assert spmv.bsr_to_csr_gpu(A, full, 0) == 0          # the CSR twin: the stored non-zeros
        spmv.bsr_destroy(full)
        del values

        status, counted = spmv.csr_block_count_gpu(A, b)
        assert status == 0 and 0 < counted <= bcols.size      # (poor_b4: a block may lose every position)
        B = spmv.bsr_create(0, 0, 2, 0)
        builds, walls = [], []
        for i in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            res = spmv.bsr_from_csr_gpu(B, A, b)
            wall = (time.perf_counter() - t0) * 1e3
            assert res.error_code == 0 and res.num_blocks == counted
            if i >= args.warmup:
                builds.append((res.symbolic_ms, res.numeric_ms))
                walls.append(wall)
        nnz = A.contents.nnz

        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        d_x, d_y = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
        d_x.copyFromHost(x, n)
        csr = timed(lambda: spmv.spmv_csr(A, d_x, d_y, vector, n))
        y_csr = d_y.copyToHost(n)
        bsr = timed(lambda: spmv.spmv_bsr(B, d_x, d_y, vector, n))
        y_bsr = d_y.copyToHost(n)
        ordered = timed(lambda: spmv.spmv_bsr(B, d_x, d_y, scalar, n))
        sweep = {}
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            os.environ["SPMV_DEBUG"] = "bsr_lanes=%d" % lanes
            sweep[str(lanes)] = round(timed(lambda: spmv.spmv_bsr(B, d_x, d_y, vector, n))[0], 4)
        os.environ.pop("SPMV_DEBUG", None)

        csr_bytes = nnz * 8 + (n + 1) * 4 + n * 8
        bsr_bytes = counted * (4 * b * b + 4) + (nodes + 1) * 4 + n * 8
        scale = np.maximum(np.abs(y_csr), 1.0)
        entry = {
            "scalar_rows": n, "block_dim": b, "nnz": int(nnz), "blocks": int(counted), "fill": round(res.fill, 4),
            "break_even_fill": round(0.5 + 0.5 / (b * b), 4), "lanes": res.lanes,
            "spmv_csr_vector_ms": round(csr[0], 4), "spmv_csr_vector_min_max_ms": [round(csr[1], 4), round(csr[2], 4)],
            "spmv_bsr_vector_ms": round(bsr[0], 4), "spmv_bsr_vector_min_max_ms": [round(bsr[1], 4), round(bsr[2], 4)],
            "spmv_bsr_ordered_ms": round(ordered[0], 4),
            "csr_model_gb_s": round(csr_bytes / 1e6 / csr[0], 1), "bsr_model_gb_s": round(bsr_bytes / 1e6 / bsr[0], 1),
            "speedup_bsr_over_csr": round(csr[0] / bsr[0], 3), "byte_ratio_csr_over_bsr": round(csr_bytes / bsr_bytes, 3),
            "fraction_of_byte_ratio": round((csr[0] / bsr[0]) / (csr_bytes / bsr_bytes), 3),
            "spmv_bsr_vector_ms_by_forced_lanes": sweep,
            "build_symbolic_ms": round(statistics.median(s for s, _ in builds), 4),
            "build_numeric_ms": round(statistics.median(v for _, v in builds), 4),
            "build_wall_ms": round(statistics.median(walls), 4),
            "build_device_ms_in_spmv_csr_calls": round(statistics.median(s + v for s, v in builds) / csr[0], 2),
            "build_wall_ms_in_spmv_csr_calls": round(statistics.median(walls) / csr[0], 2),
            "max_scaled_difference_of_the_two_results": float(np.max(np.abs(y_csr - y_bsr) / scale)),
        }
        print(name, json.dumps(entry), flush=True)
        report["cases"][name] = entry
        d_x.release()
        d_y.release()
        spmv.csr_destroy(A)
        spmv.bsr_destroy(B)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
