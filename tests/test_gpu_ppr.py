"""pagerank_personalized / pagerank_personalized_seeds (include/spmv/pagerank.h) on the device.

Three references, all held to the BIT unless a test says otherwise:
  * the integer prover of tests/ppr_cases.py on dyadic graphs (ranks and the reported residual), at every lane count,
    every window shape and past the grid cap;
  * the k = 1 call on the same column (column independence): ranks, iterations, residual, converged;
  * pagerank() on the direct kernels for a uniform column with n a power of two (a child process: SPMV_TILED is read
    once).
On top of that the layouts (leading dimensions, views 4 bytes past a 16-byte boundary, poisoned padding, V unchanged),
columns that freeze at different steps and parities, the float64 iteration on a power-law graph (1e-5 relative, the
bound tests/test_gpu_pagerank.py uses), the device-side rejections, the seeds entry point, repeatability, isolation
from the matrix's caches and a C++ caller."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_data as ed
import ppr_cases as pc
from array_views import SENTINEL, View
from conftest import ROOT

pytestmark = pytest.mark.gpu

POISON = SENTINEL.view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fields(r):
    return (r.error_code, r.iterations, r.converged, int(np.float32(r.final_residual).view(np.uint32)))


class Device:
    """A graph on the device, the k = 1 call on one column as the reference and the batched call in any layout."""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n = gpu, n
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self._single = {}

    def run(self, V, ldv=None, ldr=None, offset=0, damping=pc.DAMPING, tolerance=0.0, max_iterations=100):
        """(results, R) of pagerank_personalized on the n x k array V, stored with the given leading dimensions in views
        `offset` floats past a 16-byte boundary.  R is poison beforehand; asserts that its padding columns, both views'
        surroundings and V itself come back bit for bit."""
        n, k = V.shape
        ldv, ldr = ldv or k, ldr or k
        hv = np.full((n, ldv), POISON, np.float32)
        hv[:, :k] = V
        hr = np.full((n, ldr), POISON, np.float32)
        vv = View(self.gpu, hv.ravel(), offset, SENTINEL)
        vr = View(self.gpu, hr.ravel(), offset, SENTINEL)
        try:
            results = self.gpu.pagerank_personalized(self.A, vv.ptr, vr.ptr, k, ldv, ldr,
                                                     self.gpu.PageRankConfig(damping, tolerance, max_iterations))
            got = vr.download().reshape(n, ldr)
            vv.check_guards("V")
            vr.check_guards("R")
            assert np.array_equal(bits(vv.download()), bits(hv.ravel())), "V was written"
            assert np.array_equal(bits(got[:, k:]), bits(hr[:, k:])), "R's padding columns were written"
            assert len(results) == k and len({r.elapsed_ms for r in results}) == 1
            return results, got[:, :k].copy()
        finally:
            vv.release()
            vr.release()

    def single(self, v, key, **cfg):
        """(result, ranks) of the k = 1 call on one column, kept under `key`."""
        key = (key, tuple(sorted(cfg.items())))
        if key not in self._single:
            results, R = self.run(np.ascontiguousarray(v, np.float32).reshape(-1, 1), **cfg)
            self._single[key] = (results[0], R[:, 0].copy())
        return self._single[key]

    def close(self):
        self.gpu.csr_destroy(self.A)


def assert_columns_equal_their_own_call(dev, V, results, R, keys, what, **cfg):
    for j in range(V.shape[1]):
        ref, r_ref = dev.single(V[:, j], keys[j], **cfg)
        assert fields(results[j]) == fields(ref), (what, "column", j, fields(results[j]), fields(ref))
        bad = np.flatnonzero(bits(R[:, j]) != bits(r_ref))
        assert bad.size == 0, (what, "column", j, "rows", bad[:8], R[bad[:8], j], r_ref[bad[:8]])


def assert_proven(results, R, trajectories, steps, what):
    """Every column against the integer result after `steps` steps: the ranks and the reported residual to the bit."""
    for j, t in enumerate(trajectories):
        ranks, _, reported = t[steps - 1]
        r = results[j]
        assert (r.error_code, r.iterations, r.converged) == (0, steps, 0), (what, j, r.error_code, r.iterations)
        bad = np.flatnonzero(bits(R[:, j]) != bits(ranks))
        assert bad.size == 0, (what, "column", j, "rows", bad[:8], R[bad[:8], j], ranks[bad[:8]])
        got = np.float32(r.final_residual)
        assert got.view(np.uint32) == reported.view(np.uint32), (what, "column", j, "residual", got, reported)


# ------------------------------------------------------------------------------------------ 1. exact, every lane count
@pytest.mark.parametrize("lanes", ed.LANES)
@pytest.mark.parametrize("degrees", pc.DEGREES, ids=lambda d: "deg" + "_".join(map(str, d)))
def test_exact_at_every_lane_count(gpu, monkeypatch, degrees, lanes):
    """ppr_step_kernel<L, 8, 1> for every L on the four 2 048-node dyadic graphs, k = 5 (a node, a dangling node, a
    hub, a pair, eight nodes): after the proven number of steps, after one and after two (the dangling mass the device
    accumulated in step 1 enters step 2) every column is the integer result and reports the prover's residual."""
    rp, ci, va = pc.graph(degrees)
    steps, trajectories = pc.proven(degrees)
    assert steps >= pc.FLOORS[degrees]
    V = pc.teleport_matrix(pc.N, pc.seed_sets())
    dev = Device(gpu, pc.N, rp, ci, va)
    try:
        monkeypatch.setenv("SPMV_DEBUG", "ppr_lanes=%d" % lanes)
        for count in (steps, 1, 2):
            results, R = dev.run(V, max_iterations=count)
            assert_proven(results, R, trajectories, count, (degrees, lanes, count))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 2. every window shape
ALL_K = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32)


def window_sets(count):
    """The catalogue's five sets, then one-hot seeds 37 nodes apart (column j is the same whatever k)."""
    return (pc.seed_sets() + [[20 + 37 * j] for j in range(5, count)])[:count]


@pytest.mark.parametrize("k", ALL_K)
def test_every_window_shape(gpu, k):
    """(W, NW, groups) = (4, 1, 1) up to k = 4, (8, 1, 1) to 8, (8, 2, 1) to 16, (8, 2, 2) beyond, with a last window
    that is full (4, 8, 16, 32), holds one column (5, 9, 17) or lacks one (3, 7, 31): every column against the prover
    and against its own k = 1 call."""
    degrees = (4, 8)
    rp, ci, va = pc.graph(degrees)
    sets = window_sets(k)
    steps, trajectories = pc.proven(degrees, sets=window_sets(32))
    assert steps >= 4
    V = pc.teleport_matrix(pc.N, sets)
    dev = Device(gpu, pc.N, rp, ci, va)
    try:
        results, R = dev.run(V, max_iterations=steps)
        assert_proven(results, R, trajectories[:k], steps, ("windows", k))
        assert_columns_equal_their_own_call(dev, V, results, R, list(range(k)), ("windows", k), max_iterations=steps)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 3. layouts
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("ldv,ldr", [(5, 5), (6, 6), (8, 8), (6, 12)])
def test_leading_dimensions_and_alignment(gpu, ldv, ldr, offset):
    """k = 5: dwordx4 slices of V only at ldv = 8 with offset 0 and only for columns 0..3; guarded scalar loads
    everywhere else.  Device.run asserts the poison in R's padding columns and around both arrays, and V itself.  The
    columns converge at a tolerance here (their own counts), so the stop rule is compared as well."""
    degrees = (2, 4)
    rp, ci, va = pc.graph(degrees)
    V = pc.teleport_matrix(pc.N, pc.seed_sets())
    V[:, 4] = np.random.default_rng(4).uniform(0.0, 1.0, pc.N).astype(np.float32) / np.float32(1000.0)   # dense, sum near 1
    dev = Device(gpu, pc.N, rp, ci, va)
    try:
        cfg = dict(damping=0.85, tolerance=1e-5, max_iterations=200)
        results, R = dev.run(V, ldv=ldv, ldr=ldr, offset=offset, **cfg)
        assert all(r.error_code == 0 and r.converged for r in results)
        assert_columns_equal_their_own_call(dev, V, results, R, list(range(5)), ("layout", ldv, ldr, offset), **cfg)
        assert np.all(np.abs(R.astype(np.float64).sum(axis=0) - 1.0) < 1e-5)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 4. reduces to pagerank()
@pytest.mark.parametrize("n", [2048, 4096])
def test_a_uniform_column_is_pagerank_on_the_direct_kernels(gpu, n):
    """tests/ppr_pagerank_worker.py in a fresh process under SPMV_TILED=0 (the variable is read once): non-dyadic
    graphs, damping 0.85, tolerance 1e-6, k = 3 with column 1 = 1 / n between two seeded columns; column 1 must equal
    pagerank() in ranks, iterations, residual and converged."""
    env = dict(os.environ, SPMV_TILED="0")
    env.pop("SPMV_DEBUG", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ppr_pagerank_worker.py"), str(n)], env=env,
                         capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "column 1 equals pagerank()" in out.stdout, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------ 5. freezing
def test_columns_freeze_on_their_own(gpu):
    """A non-dyadic graph, damping 0.85, tolerance 1e-6.  A seed on a dangling node converges in its first step
    (A v = 0 and s = 1 give r = v back), the others take their own numbers of steps.  Two columns that converge on
    opposite step parities (picked from the k = 1 counts) rest in different rank arrays when the loop ends: both must
    arrive in R.  Then a max_iterations between the counts stops the slow columns unconverged."""
    pagerank_tests = importlib.import_module("test_gpu_pagerank")
    n = 4096
    rp, ci, va = pagerank_tests.graph(gpu, n, 6, 31, dangling=(5, 1000, 3000))
    dev = Device(gpu, n, rp, ci, va)
    try:
        cfg = dict(damping=0.85, tolerance=1e-6, max_iterations=100)
        hub = int(np.argmax(np.diff(rp)))
        candidates = [[5], [hub], [17], [17, 900], list(range(0, n, n // 8)), list(range(n)), [2000], [77, 78, 79, 80]]
        V_all = pc.teleport_matrix(n, candidates)
        counts = [dev.single(V_all[:, j], ("freeze", j), **cfg)[0].iterations for j in range(len(candidates))]
        print("k = 1 iteration counts", counts)
        assert counts[0] == 1 and max(counts) >= counts[0] + 4
        odd = next(j for j in range(1, len(counts)) if counts[j] % 2 == 1)
        even = next(j for j in range(1, len(counts)) if counts[j] % 2 == 0)
        slowest = int(np.argmax(counts))
        pick = list(dict.fromkeys([0, odd, even, slowest, 1, 2, 5, 6]))       # six or more: one window of eight
        V = np.ascontiguousarray(V_all[:, pick])
        results, R = dev.run(V, **cfg)
        assert [r.iterations for r in results] == [counts[j] for j in pick] and all(r.converged for r in results)
        assert_columns_equal_their_own_call(dev, V, results, R, [("freeze", j) for j in pick], "freeze", **cfg)
        assert np.array_equal(bits(R[:, 0]), bits(V[:, 0]))                 # the dangling seed: r = v
        cut = (min(counts[1:]) + max(counts)) // 2
        assert min(counts[1:]) <= cut < max(counts)
        short = dict(cfg, max_iterations=cut)
        results, R = dev.run(V, **short)
        assert [r.iterations for r in results] == [min(counts[j], cut) for j in pick]
        assert [r.converged for r in results] == [int(counts[j] <= cut) for j in pick]
        assert not all(r.converged for r in results)
        assert_columns_equal_their_own_call(dev, V, results, R, [("freeze", j) for j in pick], "cut", **short)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. past the grid cap
TRIPS = [(1 << 20, 1), (1 << 14, 64)]


@pytest.mark.parametrize("n,lanes", TRIPS, ids=["n%d_L%d" % t for t in TRIPS])
def test_exact_past_the_grid_cap(gpu, monkeypatch, n, lanes):
    """Out-degrees (1, 2): L = 1 on its own at n = 2^20 (the cap is 2 048 workgroups x 256 rows: the grid-stride loop
    goes round twice), forced L = 64 at n = 2^14 (4 rows per workgroup: two trips).  k = 4 one-hot seeds, two of them
    in rows of the second trip; the prover's count is asserted, nothing is skipped."""
    rng = np.random.default_rng(n)
    rp, ci, va = ed.dyadic_graph(rng, n, (1, 2), ed.DYADIC_DIRECT_DANGLING, [(n // 3, 1500), (n - 1, 600)])
    assert ed.lanes_for(len(ci), n) == 1
    rows_per_trip = 2048 * (256 // lanes)
    assert rows_per_trip < n <= 2 * rows_per_trip
    sets = [[7], [n // 3], [rows_per_trip + 3], [n - 2]]
    steps, trajectories = pc.proven(None, sets=sets, n=n, graph_arrays=(rp, ci, va), max_steps=4)
    print("n", n, "lanes", lanes, "exact steps", steps)
    assert steps >= 2
    V = pc.teleport_matrix(n, sets)
    dev = Device(gpu, n, rp, ci, va)
    try:
        if lanes != 1:
            monkeypatch.setenv("SPMV_DEBUG", "ppr_lanes=%d" % lanes)
        for count in (steps, 1):
            results, R = dev.run(V, max_iterations=count)
            assert_proven(results, R, trajectories, count, (n, lanes, count))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 7. general graphs
def test_power_law_graph_against_the_float64_iteration(gpu):
    """About 20 000 nodes, power-law in-degrees, column-stochastic, a few dangling nodes; k = 3: a one-hot seed, a set
    of sixteen, a dense random distribution.  Every rank within 1e-5 relative of the float64 iteration at equal step
    counts (tests/test_gpu_pagerank.py's bound for the same comparison; nodes no seed reaches are 0 on both sides);
    iteration counts equal, or one apart where the reference residual is within 1e-3 relative of the tolerance."""
    n = 20_011
    lens = gpu.synth.power_law_lengths(5, n, n_cols=n)
    rp, ci, _ = gpu.synth.stratified_csr(5, 0, lens, n)
    keep = ~np.isin(ci, np.array([11, 4000, 15000], np.int32))
    counts = np.bincount(np.repeat(np.arange(n), np.diff(rp))[keep], minlength=n)
    ci = ci[keep]
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    va = gpu.synth.column_stochastic_values(ci, n)
    assert int(rp[-1]) == ci.size
    rng = np.random.default_rng(8)
    V = pc.teleport_matrix(n, [[123], list(rng.choice(n, 16, replace=False)), [0]])
    V[:, 2] = rng.uniform(0.0, 1.0, n).astype(np.float32)
    V[:, 2] /= V[:, 2].sum(dtype=np.float64).astype(np.float32)
    tol = 1e-6
    dev = Device(gpu, n, rp, ci, va)
    try:
        results, R = dev.run(V, damping=0.85, tolerance=tol, max_iterations=100)
        want, its, residuals, conv = pc.power_iteration64(rp, ci, va, n, V, 0.85, tol, 100)
        print("iterations", [r.iterations for r in results], its, "residuals", [r.final_residual for r in results],
              [h[-1] for h in residuals])
        for j, r in enumerate(results):
            assert r.error_code == 0 and r.converged and conv[j]
            if r.iterations != its[j]:                      # the step at which the two disagree: min(...), 1-based
                at = residuals[j][min(r.iterations, its[j]) - 1]
                assert abs(r.iterations - its[j]) == 1 and abs(at - tol) <= 1e-3 * tol, (j, r.iterations, its[j], at)
        same = min(min(r.iterations for r in results), min(its))
        results, R = dev.run(V, damping=0.85, tolerance=0.0, max_iterations=same)
        want, its, _, _ = pc.power_iteration64(rp, ci, va, n, V, 0.85, 0.0, same)
        assert [r.iterations for r in results] == its == [same] * 3
        err = np.abs(R.astype(np.float64) - want)
        worst = float(np.max(np.where(want > 0, err / np.where(want > 0, want, 1.0), np.where(err > 0, np.inf, 0.0))))
        print("worst relative rank error", worst, "after", same, "steps")
        assert worst <= 1e-5
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 8. device-side rejections
def test_bad_teleport_columns_are_rejected_with_r_untouched(gpu):
    """A negative entry, a NaN, an infinity and an all-zero column, each in one column of an otherwise good V, at k = 3
    and k = 9 (the second window): INVALID_ARGUMENT in every entry, R still poison (Device.run hands in a poisoned R)."""
    rp, ci, va = pc.graph((2, 4))
    dev = Device(gpu, pc.N, rp, ci, va)
    try:
        E = gpu.SpMVError
        for k, column in ((3, 1), (9, 8), (9, 0)):
            good = pc.teleport_matrix(pc.N, window_sets(k))
            for what, row, value in (("negative", 900, -0.25), ("nan", 901, np.nan), ("inf", 5, np.inf), ("zero", None, 0.0)):
                V = good.copy()
                if row is None:
                    V[:, column] = 0.0
                else:
                    V[row, column] = value
                results, R = dev.run(V, ldr=k + 1, max_iterations=3)
                assert [r.error_code for r in results] == [E.INVALID_ARGUMENT] * k, (k, column, what)
                assert all((r.iterations, r.converged) == (0, 0) for r in results)
                assert np.all(bits(R) == SENTINEL), (k, column, what)
            results, _ = dev.run(good, max_iterations=1)
            assert all(r.error_code == 0 for r in results)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 9. the seeds entry point
def test_seed_sets_equal_the_explicit_teleport_matrix(gpu):
    """pagerank_personalized_seeds builds V with value 1.0f / count: the same bits as teleport_matrix's, so the two
    calls agree bit for bit; ldr with padding; a node may sit in two different sets."""
    degrees = (4, 8)
    rp, ci, va = pc.graph(degrees)
    sets = pc.seed_sets() + [[17, 3, 1000], [5, 6, 7, 8, 9, 10, 11]]      # counts 3 and 7: 1 / count is rounded
    V = pc.teleport_matrix(pc.N, sets)
    k = len(sets)
    dev = Device(gpu, pc.N, rp, ci, va)
    d_R = gpu.CudaBuffer(pc.N * (k + 2))
    try:
        cfg = dict(damping=0.85, tolerance=1e-6, max_iterations=40)
        want_results, want = dev.run(V, **cfg)
        d_R.copyFromHost(np.full(pc.N * (k + 2), POISON, np.float32), pc.N * (k + 2))
        results = gpu.pagerank_personalized_seeds(dev.A, sets, d_R, ldr=k + 2, config=gpu.PageRankConfig(0.85, 1e-6, 40))
        got = d_R.copyToHost(pc.N * (k + 2)).reshape(pc.N, k + 2)
        assert [fields(r) for r in results] == [fields(r) for r in want_results]
        assert np.array_equal(bits(got[:, :k]), bits(want)) and np.all(bits(got[:, k:]) == SENTINEL)
    finally:
        d_R.release()
        dev.close()


# ------------------------------------------------------------------------------------------ 10. repeatability, isolation
def test_same_bits_on_every_run_and_no_trace_in_the_matrix_caches(gpu):
    """Two calls, a call after csr_invalidate_gpu_cache and a call after a pagerank() on the same matrix (which
    caches its own workspace and mask there) give the same bits; on a tiled-eligible matrix the call builds no plan
    and leaves the promotion count alone (VECTOR_CSR calls promote afterwards exactly as on a fresh matrix)."""
    pagerank_tests = importlib.import_module("test_gpu_pagerank")
    n = 1 << 17
    rp, ci, va = pagerank_tests.graph(gpu, n, 10, 3, dangling=(5, 1000, 100_000))
    assert gpu.tiled_shape(n, n, ci.size)[0]
    dev = Device(gpu, n, rp, ci, va)
    saved = gpu.get_tiled_promotion()
    try:
        gpu.set_tiled_promotion(2)
        rng = np.random.default_rng(12)
        V = pc.teleport_matrix(n, [[9], list(rng.choice(n, 64, replace=False)), [5], list(range(n)), [77, 78]])
        cfg = dict(damping=0.85, tolerance=1e-6, max_iterations=12)
        first, R1 = dev.run(V, **cfg)
        assert all(r.error_code == 0 for r in first) and len({r.iterations for r in first}) > 1
        again, R2 = dev.run(V, **cfg)
        gpu.csr_invalidate_gpu_cache(dev.A)
        third, R3 = dev.run(V, **cfg)
        assert gpu.csr_tiled_info(dev.A) is None and not gpu.csr_has_tiled_plan(dev.A)
        r = gpu.pagerank(dev.A, gpu.PageRankConfig(0.85, 1e-6, 3))         # three direct steps: no plan yet
        assert r.iterations == 3 and not gpu.csr_has_tiled_plan(dev.A)
        fourth, R4 = dev.run(V, **cfg)
        for results, R in ((again, R2), (third, R3), (fourth, R4)):
            assert [fields(x) for x in results] == [fields(x) for x in first]
            assert np.array_equal(bits(R), bits(R1))
        assert gpu.csr_tiled_info(dev.A) is None
        d_x, d_y = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        d_x.copyFromHost(np.ascontiguousarray(V[:, 3]), n)
        for call in range(3):
            assert gpu.spmv_csr(dev.A, d_x, d_y, gpu.SpMVConfig(1), n).error_code == 0
            assert gpu.csr_has_tiled_plan(dev.A) == (call >= 2), call
        d_x.release()
        d_y.release()
    finally:
        gpu.set_tiled_promotion(saved)
        dev.close()


# ------------------------------------------------------------------------------------------ 11. C++ caller
def test_cpp_ppr_smoke(gpu, tmp_path):
    """tests/cpp/ppr_smoke.cpp through spmv/pagerank.h and CudaBuffer, compiled here with test_cpp_cg_smoke's g++ line."""
    exe = str(tmp_path / "ppr_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "ppr_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
