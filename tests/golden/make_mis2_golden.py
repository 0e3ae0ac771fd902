"""make_mis2_golden.py — regenerates tests/golden/mis2_restate.json.

Runs tests/mis2_cases.py's numpy restatement of the MIS-2 aggregation (include/spmv/amg.h) at seed 0 and the default
AMGConfig on the matrices of mis2_cases.SIZED: the rows of every level of the restated hierarchy, the synchronous
round count of every aggregated level, and the step count of the fp32 restated PCG to 1e-6 (test_gpu_cg_ic.restate_ic
with amg_cases.vcycle as the preconditioner).  The Galerkin products are spgemm_cpu_csr's, on the host: no GPU is
needed, the library must be built.  tests/test_amg_mis2_host.py checks the file against a fresh run.

usage:  python tests/golden/make_mis2_golden.py
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mis2_cases as mc  # noqa: E402


def main():
    spmv = importlib.import_module("gpu-spmv_amd")
    out = {name: mc.restated(spmv, name)[0] for name in mc.SIZED}
    with open(mc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
