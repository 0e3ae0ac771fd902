"""bsr_view_bench.py — spmv_bsr VECTOR_CSR at b = 8 on a value array that is 16-byte aligned and on the same values as
a view 4 bytes past a 16-byte boundary (bsr_wrap_device): the two load forms of bsr_lanes_kernel<8, LANES, WIDE>, at
the natural lane count and at every forced one.  The dword form (WIDE = false) is the one whose register count moved
when the block-row walk became a device function, so this is run on the library before and after
that change (SPMV_AMD_LIB, or a second checkout) and both outputs are kept in profiles/bsr_view_bench.json.

Matrix: 3-D 7-point stencil on 48^3 nodes, full 8x8 blocks, values uniform in [-1, 1] (884 736 scalar rows).  Medians
and min - max over --runs calls after --warmup of elapsed_ms (device events inside the call).

    python tools/bsr_view_bench.py [--runs 20] [--warmup 3] [--label after] [--out FILE]
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bsr_bench import stencil_blocks  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="after")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    spmv = importlib.import_module("gpu-spmv_amd")
    spmv.require_gpu()
    spmv.set_tiled_promotion(0)
    os.environ.pop("SPMV_DEBUG", None)
    vector = spmv.SpMVConfig(kernel_type=spmv.SpMVConfig.VECTOR_CSR, use_texture=False)

    b = 8
    nodes, brp, bcols = stencil_blocks((48, 48, 48), "cross")
    n = nodes * b
    rng = np.random.default_rng(8)
    values = rng.uniform(-1.0, 1.0, size=bcols.size * b * b).astype(np.float32)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)

    d_rp, d_bc = spmv.CudaBuffer(brp.size, "int32"), spmv.CudaBuffer(bcols.size, "int32")
    d_rp.copyFromHost(brp, brp.size)
    d_bc.copyFromHost(bcols, bcols.size)
    d_va = spmv.CudaBuffer(values.size + 8)                  # room for the payload at either offset
    d_x, d_y = spmv.CudaBuffer(n), spmv.CudaBuffer(n)
    d_x.copyFromHost(x, n)
    assert d_va.get() % 16 == 0

    def timed(B):
        times = []
        for i in range(args.warmup + args.runs):
            res = spmv.spmv_bsr(B, d_x, d_y, vector, n)
            if res.error_code != 0:
                raise RuntimeError(spmv.spmv_error_string(res.error_code))
            if i >= args.warmup:
                times.append(res.elapsed_ms)
        return [round(statistics.median(times), 4), round(min(times), 4), round(max(times), 4)]

    report = {"label": args.label, "device": spmv.device_name(), "scalar_rows": n, "block_dim": b,
              "blocks": int(bcols.size), "runs": args.runs, "warmup": args.warmup}
    results = {}
    for name, offset in (("aligned_16_byte_loads", 0), ("view_at_4_bytes_dword_loads", 1)):
        padded = np.zeros(values.size + 8, np.float32)
        padded[offset:offset + values.size] = values
        d_va.copyFromHost(padded, padded.size)
        B = spmv.bsr_wrap_device(n, n, b, int(bcols.size), d_rp.get(), d_bc.get(), d_va.get() + 4 * offset)
        entry = {"natural_lanes_ms": timed(B)}
        results[name + "_y"] = d_y.copyToHost(n)
        for lanes in (1, 2, 4, 8, 16, 32, 64):
            os.environ["SPMV_DEBUG"] = "bsr_lanes=%d" % lanes
            entry["lanes_%d_ms" % lanes] = timed(B)
        os.environ.pop("SPMV_DEBUG", None)
        report[name] = entry
        spmv.bsr_destroy(B)
    report["same_bits_in_both_forms"] = bool(np.array_equal(results["aligned_16_byte_loads_y"].view(np.uint32),
                                                            results["view_at_4_bytes_dword_loads_y"].view(np.uint32)))
    print(json.dumps(report), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
