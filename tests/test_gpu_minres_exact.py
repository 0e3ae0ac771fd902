"""minres_solve / minres_solve_ic held to the bit on the exact families of tests/minres_cases.py, past the grid caps.

On these systems every scalar and every vector entry of the first two steps is a dyadic rational that fp32 holds
(tests/test_minres_host.py proves it in integer / Fraction arithmetic), so every summation order -- the device's lanes
and workgroup partials, either engine -- must give the restatement's bits: x, iterations, converged, breakdown and
relative_residual after max_iterations = 1 and = 2 at zero tolerance, and true_relative_residual == 0 once x = A^-1 b.
The sizes are exact_data's: TRIP_SIZES make every grid-stride loop of the element-wise kernels and of the one-lane row
kernels take a second trip, LANE_SIZES reach every lanes-per-row instantiation past its own row trip, and
TILED_TRIP_SIZE runs on the tiled engine."""
import numpy as np
import pytest

import exact_data as ed
import minres_cases as mc

pytestmark = pytest.mark.gpu

TILED_SMALL = "min_cols=1,min_nnz=1"
SIZES = [(n, 1) for n in ed.TRIP_SIZES] + [(n, L) for L, n in ed.LANE_SIZES.items()]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _run(gpu, system, engines):
    n = system["n"]
    A = gpu.csr_from_arrays(n, n, system["rp"], system["ci"], system["va"])
    assert gpu.csr_to_gpu(A) == 0
    d_b, d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_b.copyFromHost(system["b"], n)
    F = None
    try:
        for kind in mc.exact_preconditioners(system["family"]):
            if kind == "ic" and F is None:
                F = gpu.csr_from_arrays(n, n, *mc.exact_factor(n))
                assert gpu.csr_to_gpu(F) == 0
            for steps in (1, 2):
                x_ref, it, conv, brk, rel = mc.exact_reference(system, kind, steps)
                for engine in engines:
                    cfg = gpu.MinresConfig(tolerance=0.0, max_iterations=steps, engine=engine, shift=system["shift"],
                                           preconditioner=mc.JACOBI if kind == "jacobi" else mc.NONE)
                    d_x.copyFromHost(np.zeros(n, np.float32), n)
                    res = gpu.minres_solve_ic(A, F, d_b, d_x, cfg) if kind == "ic" else \
                        gpu.minres_solve(A, d_b, d_x, cfg)
                    what = (system["family"], n, system["L"], kind, steps, engine)
                    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, it, int(conv), brk), \
                        (what, res.iterations, res.converged, res.breakdown)
                    assert bits(res.relative_residual) == bits(np.float32(rel)), (what, res.relative_residual, rel)
                    x = d_x.copyToHost(n)
                    wrong = np.flatnonzero(bits(x) != bits(x_ref))
                    assert wrong.size == 0, (what, wrong[:8], x[wrong[:8]], x_ref[wrong[:8]])
                    if conv:
                        assert res.true_relative_residual == 0.0, what
                    assert gpu.csr_has_tiled_plan(A) == (engine == 1), what
    finally:
        if F is not None:
            gpu.csr_destroy(F)
        gpu.csr_destroy(A)
        d_b.release()
        d_x.release()


@pytest.mark.parametrize("family", mc.EXACT_FAMILIES)
@pytest.mark.parametrize("n,L", SIZES)
def test_exact_at_every_trip_and_lane_count(gpu, family, n, L):
    _run(gpu, mc.exact_system(family, n, L), engines=(0,))


@pytest.mark.parametrize("family", mc.EXACT_FAMILIES)
def test_exact_on_the_tiled_engine(gpu, monkeypatch, family):
    monkeypatch.setenv("SPMV_DEBUG", TILED_SMALL)               # lets the tiled engine take this matrix
    _run(gpu, mc.exact_system(family, ed.TILED_TRIP_SIZE, 1), engines=(1,))
