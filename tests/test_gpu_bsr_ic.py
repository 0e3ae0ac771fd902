"""bsr_ic0, sptrsv_bsr and cg_solve_bsr_ic (include/spmv/bsr_factor.h, include/spmv/cg.h) on the device.

Zero tolerance unless said: the device factor against bsr_ic0_cpu bit for bit at every block size x forced lane count
(float family with the dropped-fill matrix, value arrays as views at 4-, 8- and 12-byte offsets with guard words, in
place) and against the integers on the exact family; ordered solves against sptrsv_cpu_bsr; unordered solves at zero
tolerance on the exact family and under a derived bound on the float family; the launch geometry (sizes below b, one
block row, the narrow / wide boundary, the grid caps, a chain longer than one single-workgroup launch, a narrow run
before a wide level); the schedule cache; the exact one-step solves of cg_solve_bsr_ic; float systems against the
restatement under test_gpu_cg_ic.py's bounds; and the behaviour rules of cg.h.

The constants behind the sizes (csrc/device_common.h, csrc/internal.h): kBlock = 256 threads; a wide level runs on at
most kMaxResidentBlocks = 2048 workgroups of 256 / L block rows each; a level of at most kSptrsvNarrowRows = 256 block
rows is narrow, and one workgroup walks at most kSptrsvMaxRunLevels = 8192 narrow levels in a launch; cg_update_kernel
runs on at most kVecBlocks = 1024 workgroups of 256 rows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bsr_ic_cases as ic
from conftest import ROOT

pytestmark = pytest.mark.gpu

OK, DIMENSION, FORMAT, ARGUMENT = 0, -1, -5, -8
TOL = 1e-6
GUARD = np.float32(-12345.5)


def addr(p):
    return ctypes.cast(p, ctypes.c_void_p).value


class Dev:
    """A BSR matrix on the device with a factor buffer, the factor matrix F over A's structure arrays, and vectors"""

    def __init__(self, gpu, n, b, brp, bc, bv):
        self.gpu, self.n, self.b = gpu, n, b
        self.brp, self.bc, self.bv = brp, bc, np.ascontiguousarray(bv, np.float32)
        self.A = gpu.bsr_from_arrays(n, n, b, brp, bc, bv)
        assert gpu.bsr_to_gpu(self.A) == 0
        self.count = int(self.bv.size)
        self.d_f = gpu.CudaBuffer(max(self.count, 1))
        c = self.A.contents
        self.F = gpu.bsr_wrap_device(n, n, b, c.num_blocks, addr(c.d_block_row_ptrs), addr(c.d_block_cols),
                                     self.d_f.get())
        self.d_b, self.d_x = gpu.CudaBuffer(max(n, 1)), gpu.CudaBuffer(max(n, 1))
        self.host_f = None

    def cpu_factor(self):
        if self.host_f is None:
            self.host_f, self.host_bad = self.gpu.bsr_ic0_cpu(self.A)
            self.Fh = self.gpu.bsr_from_arrays(self.n, self.n, self.b, self.brp, self.bc, self.host_f)
        return self.host_f

    def factor(self):
        res = self.gpu.bsr_ic0(self.A, self.d_f)
        assert res.error_code == 0, self.gpu.spmv_error_string(res.error_code)
        return res, self.d_f.copyToHost(self.count)

    def solve(self, rhs, in_place=False, **cfg):
        cfg = self.gpu.SpTRSVConfig(**cfg)
        self.d_x.copyFromHost(np.full(self.n, 7.0, np.float32), self.n)
        target = self.d_x if in_place else self.d_b
        target.copyFromHost(np.ascontiguousarray(rhs, np.float32), self.n)
        res = self.gpu.sptrsv_bsr(self.F, target, self.d_x, cfg)
        return res, self.d_x.copyToHost(self.n)

    def cg(self, rhs, x0=None, **cfg):
        x0 = np.zeros(self.n, np.float32) if x0 is None else np.asarray(x0, np.float32)
        self.d_b.copyFromHost(np.ascontiguousarray(rhs, np.float32), self.n)
        self.d_x.copyFromHost(x0, self.n)
        res = self.gpu.cg_solve_bsr_ic(self.A, self.F, self.d_b, self.d_x, self.gpu.CGConfig(**cfg))
        return res, self.d_x.copyToHost(self.n)

    def close(self):
        self.gpu.bsr_destroy(self.F)
        if self.host_f is not None:
            self.gpu.bsr_destroy(self.Fh)
        self.gpu.bsr_destroy(self.A)
        for buf in (self.d_f, self.d_b, self.d_x):
            buf.release()


def dev_of(gpu, s):
    return Dev(gpu, s["n"], s["b"], s["brp"], s["bc"], s["bv"])


# ---- the factor ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_the_factor_is_the_host_twins_at_every_lane_count(gpu, monkeypatch, b):
    for name, n, brp, bc, bv in ic.float_family(b, small=False):
        d = Dev(gpu, n, b, brp, bc, bv)
        want = d.cpu_factor()
        assert d.host_bad == -1, name
        for lanes in ic.LANES:
            ic.forced(monkeypatch, lanes)
            res, got = d.factor()
            assert res.lanes_per_row == lanes and res.bad_pivot == -1 and res.launches >= 1, (name, lanes)
            ic.assert_bits(got, want, (name, lanes))
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        res, got = d.factor()                                         # the library's own lane count
        assert res.lanes_per_row in ic.LANES
        ic.assert_bits(got, want, (name, "default lanes"))
        # in place: A's own device values
        res = gpu.bsr_ic0(d.A, addr(d.A.contents.d_values))
        assert res.error_code == 0
        assert gpu.bsr_from_gpu(d.A) == 0
        ic.assert_bits(gpu.bsr_host_arrays(d.A)[2], want, (name, "in place"))
        d.close()


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_value_arrays_that_are_views_with_guard_words(gpu, monkeypatch, b):
    import torch
    nodes, pairs = ic.grid_pattern("2d9", 7, 0.45, seed=7)
    n, brp, bc, bv = ic.laplacian_bsr(nodes, pairs, b, nodes * b - (b - 1), seed=b)
    H = gpu.bsr_from_arrays(n, n, b, brp, bc, bv)
    want, bad = gpu.bsr_ic0_cpu(H)
    gpu.bsr_destroy(H)
    t_rp, t_bc = torch.from_numpy(brp).cuda(), torch.from_numpy(bc).cuda()
    for words in (1, 2, 3):
        for lanes in (1, 4, 64):
            ic.forced(monkeypatch, lanes)
            a_buf = torch.full((bv.size + 8,), float(GUARD), dtype=torch.float32).cuda()
            f_buf = torch.full((bv.size + 8,), float(GUARD), dtype=torch.float32).cuda()
            a_buf[words:words + bv.size] = torch.from_numpy(bv).cuda()
            A = gpu.bsr_wrap_device(n, n, b, int(bc.size), t_rp.data_ptr(), t_bc.data_ptr(), a_buf.data_ptr() + 4 * words)
            res = gpu.bsr_ic0(A, f_buf.data_ptr() + 4 * words)
            assert res.error_code == 0 and res.bad_pivot == bad == -1
            got = f_buf.cpu().numpy()
            ic.assert_bits(got[words:words + bv.size], want, (b, words, lanes))
            assert (got[:words] == GUARD).all() and (got[words + bv.size:] == GUARD).all()
            after = a_buf.cpu().numpy()
            ic.assert_bits(after[words:words + bv.size], bv, "A is only read")
            # the solves read the factor through the same view
            F = gpu.bsr_wrap_device(n, n, b, int(bc.size), t_rp.data_ptr(), t_bc.data_ptr(), f_buf.data_ptr() + 4 * words)
            rhs = np.random.default_rng(words).uniform(-1.0, 1.0, n).astype(np.float32)
            Fh = gpu.bsr_from_arrays(n, n, b, brp, bc, want)
            x_buf = torch.full((n + 8,), float(GUARD), dtype=torch.float32).cuda()
            t_b = torch.from_numpy(rhs).cuda()
            for uplo in (0, 1):
                cfg = gpu.SpTRSVConfig(uplo=uplo, ordered=1)
                assert gpu.sptrsv_bsr(F, t_b.data_ptr(), x_buf.data_ptr() + 4 * words, cfg).error_code == 0
                x = x_buf.cpu().numpy()
                ic.assert_bits(x[words:words + n], gpu.sptrsv_cpu_bsr(Fh, rhs, None, cfg)[1], (b, words, uplo))
                assert (x[:words] == GUARD).all() and (x[words + n:] == GUARD).all()
            for M in (A, F, Fh):
                gpu.bsr_destroy(M)
    monkeypatch.delenv("SPMV_DEBUG", raising=False)


def _exact_check(gpu, monkeypatch, s, lanes_list, what, solver=True):
    """factor == the integers, both unordered solves and the one-step CG at zero tolerance"""
    d = dev_of(gpu, s)
    x, rhs = ic.exact_solution(s)
    for lanes in lanes_list:
        ic.forced(monkeypatch, lanes)
        res, got = d.factor()
        assert res.bad_pivot == -1 and res.lanes_per_row == lanes, (what, lanes)
        ic.assert_bits(got + np.float32(0.0), s["fv"], (what, lanes, "factor"))
        r1, y = d.solve(rhs, uplo=ic.LOWER)
        r2, z = d.solve(y, in_place=True, uplo=ic.UPPER)
        assert r1.error_code == r2.error_code == 0 and r1.lanes_per_row == lanes, (what, lanes)
        ic.assert_bits(z + np.float32(0.0), x + np.float32(0.0), (what, lanes, "solves"))
        if solver and rhs.any():
            res, got_x = d.cg(rhs, tolerance=TOL, max_iterations=20, engine=0)
            tag = (what, lanes, res.error_code, res.iterations, res.converged, res.relative_residual)
            assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, 1, 1, 0), tag
            assert res.relative_residual == 0.0, tag
            ic.assert_bits(got_x + np.float32(0.0), x + np.float32(0.0), tag)
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    d.close()
    return r1, r2


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_the_exact_family_at_every_lane_count(gpu, monkeypatch, b):
    cases = [("chain", ic.exact_forest(1, 40, b)), ("forest", ic.exact_forest(300, 3, b)),
             ("block diagonal", ic.exact_forest(600, 1, b))]
    for cut in range(1, b):
        cases.append(("forest cut %d" % cut, ic.exact_forest(7, 5, b, 35 * b - cut)))
    cases.append(("arrow", ic.exact_arrow(40, b, 41 * b - (b - 1))))
    for name, s in cases:
        _exact_check(gpu, monkeypatch, s, ic.LANES, (name, b))


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_bad_pivot_is_the_lowest_block_row(gpu, monkeypatch, b):
    nodes, pairs = ic.grid_pattern("2d9", 12)
    n, brp, bc, bv = ic.laplacian_bsr(nodes, pairs, b, seed=6)
    diag = ic.diagonal_positions(brp, bc)
    blocks = bv.reshape(-1, b, b).copy()
    for I in (100, 37, 90):
        blocks[diag[I], 0, 0] = -1.0
    d = Dev(gpu, n, b, brp, bc, blocks.reshape(-1))
    want = d.cpu_factor()
    assert d.host_bad == 37
    for lanes in (1, 8, 64):
        ic.forced(monkeypatch, lanes)
        res, got = d.factor()
        assert res.error_code == 0 and res.bad_pivot == 37
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(ic.bits(got)[~nan], ic.bits(want)[~nan])
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    d.close()


@pytest.mark.parametrize("b, seed, bad_pivot", ic.BREAKDOWN_SPD)
def test_a_breakdown_that_ic0_meets_by_itself_on_an_irregular_pattern(gpu, monkeypatch, b, seed, bad_pivot):
    n, brp, bc, bv = ic.block_spd_bsr(300 * b - 1, b, seed, coupling=0.9)
    d = Dev(gpu, n, b, brp, bc, bv)
    want = d.cpu_factor()
    nan = np.isnan(want)
    assert d.host_bad == bad_pivot and nan.any()
    for lanes in ic.LANES:
        ic.forced(monkeypatch, lanes)
        res, got = d.factor()
        assert (res.error_code, res.bad_pivot) == (0, bad_pivot), lanes
        assert np.array_equal(np.isnan(got), nan), lanes
        assert np.array_equal(ic.bits(got)[~nan], ic.bits(want)[~nan]), lanes
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    d.close()


def test_launch_geometry(gpu, monkeypatch):
    b = 2
    # 1, b - 1, b and b + 1 scalar rows; one block row
    for n in (1, b - 1, b, b + 1):
        nb = -(-n // b)
        s = ic.exact_forest(1, nb, b, n)
        r1, _ = _exact_check(gpu, monkeypatch, s, (1, 64), ("rows", n))
        assert r1.num_levels == nb and r1.launches == 1
    # the narrow / wide boundary: 256 chains make narrow levels (one launch), 257 wide ones (a launch per level)
    for chains, launches in ((ic.NARROW, 1), (ic.NARROW + 1, 3)):
        r1, r2 = _exact_check(gpu, monkeypatch, ic.exact_forest(chains, 3, b), (1, 16), ("forest", chains))
        assert (r1.num_levels, r1.launches, r2.launches) == (3, launches, launches)
    # a chain of kSptrsvMaxRunLevels + 3 block rows: two single-workgroup launches
    r1, r2 = _exact_check(gpu, monkeypatch, ic.exact_forest(1, ic.MAX_RUN_LEVELS + 3, b), (1, 64), "long chain",
                          solver=False)
    assert (r1.num_levels, r1.launches, r2.launches) == (ic.MAX_RUN_LEVELS + 3, 2, 2)


@pytest.mark.parametrize("lanes", (64, 1))
def test_a_level_below_at_and_above_the_grid_cap(gpu, monkeypatch, lanes):
    cap = ic.ROW_BLOCKS * ic.K_BLOCK // lanes
    for chains in (cap - 1, cap, cap + 1):
        s = ic.exact_forest(chains, 2, 2, 2 * chains * 2 - 1)
        r1, _ = _exact_check(gpu, monkeypatch, s, (lanes,), ("cap", lanes, chains), solver=chains == cap + 1)
        assert (r1.num_levels, r1.launches) == (2, 2)


def test_a_run_of_narrow_levels_before_a_wide_one(gpu, monkeypatch):
    """a path 0 - 1 - 2 and 400 leaves on node 2: levels of 1, 1, 1 and 400 block rows; IC(0) drops the leaves' fill"""
    for b in (2, 3):
        pairs = [(0, 1), (1, 2)] + [(2, k) for k in range(3, 403)]
        n, brp, bc, bv = ic.laplacian_bsr(403, sorted(pairs), b, 403 * b - 1, seed=3)
        d = Dev(gpu, n, b, brp, bc, bv)
        want = d.cpu_factor()
        rhs = np.random.default_rng(b).uniform(-1.0, 1.0, n).astype(np.float32)
        for lanes in (1, 4, 64):
            ic.forced(monkeypatch, lanes)
            res, got = d.factor()
            assert (res.num_levels, res.launches) == (4, 2)
            ic.assert_bits(got, want, (b, lanes))
            for uplo in (0, 1):
                cfg = dict(uplo=uplo, ordered=1)
                r, x = d.solve(rhs, **cfg)
                assert r.error_code == 0 and r.launches == 2
                ic.assert_bits(x, gpu.sptrsv_cpu_bsr(d.Fh, rhs, None, gpu.SpTRSVConfig(**cfg))[1], (b, lanes, uplo))
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        d.close()


# ---- the solves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_ordered_solves_are_the_host_twins(gpu, b):
    rng = np.random.default_rng(b)
    for name, n, brp, bc, bv in ic.float_family(b, small=False):
        d = Dev(gpu, n, b, brp, bc, bv)
        d.cpu_factor()
        d.factor()
        rhs = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for uplo in (0, 1):
            for unit in (0, 1):
                cfg = dict(uplo=uplo, diag=unit, ordered=1)
                want = gpu.sptrsv_cpu_bsr(d.Fh, rhs, None, gpu.SpTRSVConfig(**cfg))[1]
                for in_place in (False, True):
                    res, x = d.solve(rhs, in_place=in_place, **cfg)
                    assert res.error_code == 0 and res.lanes_per_row == 1, name
                    ic.assert_bits(x, want, (name, uplo, unit, in_place))
        d.close()


def solve_bound_ratio(n, b, brp, bc, fv, rhs, x, uplo):
    """max over the rows of |x - V (rhs - s)| / bound for the device's own x, s = the fp64 off-diagonal sum with that x.
    The computed s differs from s by at most gamma(len) S, S = sum |F||x| and len its number of terms, in any order and
    with or without fusing; t = fl(rhs - s) adds u |t|; the ordered diagonal step over at most b terms adds
    gamma(b) |V||t|.  So |x - V t| <= |V| (gamma(len) S + u |t|) + gamma(b) |V||t|, u = 2^-24, gamma(k) = k u / (1 - k u)."""
    u = 2.0 ** -24
    gamma = lambda k: k * u / (1.0 - k * u)
    nb = len(brp) - 1
    F = np.asarray(fv, np.float64).reshape(-1, b, b)
    xp = np.zeros(nb * b)
    xp[:n] = x
    rp = np.zeros(nb * b)
    rp[:n] = rhs
    worst = 0.0
    for I in range(nb):
        size = min(b, n - I * b)
        s = np.zeros(b)
        S = np.zeros(b)
        terms = 0
        V = None
        for p in range(brp[I], brp[I + 1]):
            J = int(bc[p])
            if J == I:
                V = np.tril(F[p]) if uplo == 0 else np.triu(F[p])
            elif (J < I) == (uplo == 0):
                s += F[p] @ xp[J * b:(J + 1) * b]
                S += np.abs(F[p]) @ np.abs(xp[J * b:(J + 1) * b])
                terms += b
        t = rp[I * b:(I + 1) * b] - s
        want = V @ t
        bound = np.abs(V) @ (gamma(terms + 1) * S + u * np.abs(t)) + gamma(b + 1) * (np.abs(V) @ np.abs(t))
        err = np.abs(xp[I * b:(I + 1) * b] - want)[:size]
        tiny = np.finfo(np.float32).tiny
        worst = max(worst, float(np.max(err / np.maximum(bound[:size], tiny))))
    return worst


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_unordered_solves_meet_the_bound_and_repeat_their_bits(gpu, monkeypatch, b):
    import torch
    rng = np.random.default_rng(b + 10)
    # one matrix of every structure, the ragged cut where the structure has one (the full sizes are the ordered
    # test's and the factor test's)
    family = ic.float_family(b, small=False)
    picked = {}
    for case in family:
        picked[case[0].split(" ")[0]] = case                         # the last cut of each structure
    assert sorted(picked) == ["2d9", "2d9-dropped", "3d27", "3d7", "block_spd"]
    for name, n, brp, bc, bv in picked.values():
        d = Dev(gpu, n, b, brp, bc, bv)
        f = d.cpu_factor()
        d.factor()
        rhs = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for uplo in (0, 1):
            for lanes in ic.LANES + (None,):
                if lanes is None:
                    monkeypatch.delenv("SPMV_DEBUG", raising=False)
                else:
                    ic.forced(monkeypatch, lanes)
                res, x = d.solve(rhs, uplo=uplo)
                assert res.error_code == 0 and res.lanes_per_row == (lanes or res.lanes_per_row), (name, lanes)
                ratio = solve_bound_ratio(n, b, brp, bc, f, rhs, x, uplo)
                print(name, "uplo", uplo, "lanes", res.lanes_per_row, "error / bound", round(ratio, 3))
                assert ratio <= 1.0, (name, uplo, lanes, ratio)
                res2, x2 = d.solve(rhs, in_place=True, uplo=uplo)
                ic.assert_bits(x2, x, (name, uplo, lanes, "second run, in place"))
        # a side stream gives the same bits
        ic.forced(monkeypatch, 8)
        _, x = d.solve(rhs, uplo=0)
        st = torch.cuda.Stream()
        t_b, out = torch.from_numpy(rhs).cuda(), torch.zeros(n, dtype=torch.float32).cuda()
        torch.cuda.synchronize()
        assert gpu.sptrsv_bsr_async(d.F, t_b.data_ptr(), out.data_ptr(), gpu.SpTRSVConfig(uplo=0), st.cuda_stream) == 0
        torch.cuda.synchronize()
        ic.assert_bits(out.cpu().numpy(), x, (name, "side stream"))
        t_f = torch.zeros(d.count, dtype=torch.float32).cuda()
        assert gpu.bsr_ic0_async(d.A, t_f.data_ptr(), st.cuda_stream) == 0
        torch.cuda.synchronize()
        ic.assert_bits(t_f.cpu().numpy(), f, (name, "factor on a side stream"))
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        d.close()


def test_the_schedule_is_cached_shared_with_the_factor_and_dropped(gpu, monkeypatch):
    b = 3
    name, n, brp, bc, bv = ic.float_family(b, small=False)[0]
    d = Dev(gpu, n, b, brp, bc, bv)
    first = gpu.bsr_ic0(d.A, d.d_f)
    assert first.error_code == 0 and first.analysis_ms > 0
    assert gpu.bsr_ic0(d.A, d.d_f).analysis_ms == 0
    rhs = np.ones(n, np.float32)
    low, x_host = d.solve(rhs, uplo=0, ordered=1)
    assert low.error_code == 0 and low.analysis_ms == 0                 # F after A: the same structure arrays
    up, _ = d.solve(rhs, uplo=1)
    assert up.analysis_ms > 0 and d.solve(rhs, uplo=1)[0].analysis_ms == 0
    assert gpu.sptrsv_analyze_bsr(d.A, 1).analysis_ms == 0
    gpu.bsr_invalidate_gpu_cache(d.A)
    again = gpu.sptrsv_analyze_bsr(d.F, 0)
    assert again.error_code == 0 and again.analysis_ms > 0
    assert (again.num_levels, again.launches) == (first.num_levels, first.launches)
    # the device analysis: the same levels, launches and bits
    gpu.bsr_invalidate_gpu_cache(d.A)
    monkeypatch.setenv("SPMV_DEBUG", "sptrsv_analysis=device")
    on_device = gpu.bsr_ic0(d.A, d.d_f)
    assert on_device.analysis_ms > 0
    assert (on_device.num_levels, on_device.launches) == (first.num_levels, first.launches)
    ic.assert_bits(d.d_f.copyToHost(d.count), d.cpu_factor(), "device analysis")
    low2, x_dev = d.solve(rhs, uplo=0, ordered=1)
    assert (low2.num_levels, low2.launches) == (low.num_levels, low.launches)
    ic.assert_bits(x_dev, x_host, "device analysis, solve")
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    # a rebuild into an existing matrix drops the entry with the arrays
    assert gpu.bsr_to_gpu(d.A) == 0
    gpu.bsr_destroy(d.F)
    c = d.A.contents
    d.F = gpu.bsr_wrap_device(n, n, b, c.num_blocks, addr(c.d_block_row_ptrs), addr(c.d_block_cols), d.d_f.get())
    assert gpu.bsr_ic0(d.A, d.d_f).analysis_ms > 0
    d.close()


def test_the_device_analysis_rejects_what_the_host_analysis_rejects(gpu, monkeypatch):
    b = 2
    nodes, pairs = ic.grid_pattern("2d9", 4)
    n, brp, bc, bv = ic.laplacian_bsr(nodes, pairs, b, seed=2)
    blocks = bv.reshape(-1, b, b)
    keep = np.ones(bc.size, bool)
    keep[1] = False                                                   # (0, J) dropped, (J, 0) kept: one-sided
    brp_m = brp.copy()
    brp_m[1:] -= 1
    swapped = bc.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    bad_col = bc.copy()
    bad_col[1] = nodes
    for mode in ("", "sptrsv_analysis=device"):
        monkeypatch.setenv("SPMV_DEBUG", mode)
        for arrays, want in (((brp_m, bc[keep], blocks[keep].reshape(-1)), ARGUMENT), ((brp, swapped, bv), ARGUMENT),
                             ((brp, bad_col, bv), FORMAT)):
            d = Dev(gpu, n, b, *arrays)
            d.d_f.copyFromHost(np.full(d.count, 3.0, np.float32), d.count)
            assert gpu.bsr_ic0(d.A, d.d_f).error_code == want, (mode, want)
            assert (d.d_f.copyToHost(d.count) == 3.0).all()
            if arrays[1] is swapped:
                # unsorted block rows: a NON_UNIT solve and the solver say so, d_x untouched; a UNIT solve runs
                rhs = np.ones(n, np.float32)
                for uplo in (0, 1):
                    res, x = d.solve(rhs, uplo=uplo)
                    assert res.error_code == ARGUMENT and (x == 7.0).all(), (mode, uplo)
                    assert d.solve(rhs, uplo=uplo, diag=1)[0].error_code == OK
                res, x = d.cg(rhs, x0=np.full(n, 0.5, np.float32))
                assert res.error_code == ARGUMENT and (x == 0.5).all(), mode
            d.close()
    monkeypatch.delenv("SPMV_DEBUG", raising=False)


# ---- the solver ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("update cap", "solve cap"))
def test_exact_one_step_solves_around_the_grid_caps(gpu, monkeypatch, case):
    b = 2
    if case == "update cap":                                          # 1024 x 256 rows a trip of cg_update_kernel
        chains = 1024 * 256 // (2 * b)
        for s in (ic.exact_forest(chains, 2, b, 2 * chains * b - 1), ic.exact_forest(chains, 2, b),
                  ic.exact_forest(chains + 1, 2, b, 2 * (chains + 1) * b - 1)):
            _exact_check(gpu, monkeypatch, s, (4,), (case, s["n"]))
    else:                                                             # 2048 x 256 / 64 block rows a trip of a level
        cap = ic.ROW_BLOCKS * ic.K_BLOCK // 64
        for chains in (cap - 1, cap, cap + 1):
            _exact_check(gpu, monkeypatch, ic.exact_forest(chains, 2, b), (64,), (case, chains))


def true_residual(A64, rhs, x):
    b64 = np.asarray(rhs, np.float64)
    return float(np.linalg.norm(b64 - A64 @ np.asarray(x, np.float64)) / np.linalg.norm(b64))


@pytest.mark.parametrize("b", ic.BLOCK_DIMS)
def test_float_systems_against_the_restatement(gpu, b):
    """test_gpu_cg_ic.py's bounds: converged, no breakdown, the true residual within max(4 tol, twice the
    restatement's), and the same bits from a second solve"""
    for name, n, brp, bc, bv, rhs, tol in ic.parity_systems(b):
        d = Dev(gpu, n, b, brp, bc, bv)
        f = d.cpu_factor()
        d.factor()
        A64 = ic.expand(n, b, brp, bc, bv)
        x_ref, it_ref, conv_ref, brk_ref, rel_ref = ic.restate_cg(A64, rhs, tol, ic.ic_apply(n, b, brp, bc, f))
        assert conv_ref and not brk_ref
        res, x = d.cg(rhs, tolerance=tol, engine=0, preconditioner=77)
        print(name, "device steps", res.iterations, "restatement", it_ref, "rel", res.relative_residual, rel_ref)
        assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
        assert res.converged == 1 and res.breakdown == 0
        assert true_residual(A64, rhs, x) <= max(4 * tol, 2 * true_residual(A64, rhs, x_ref))
        assert abs(res.iterations - it_ref) <= 2 and res.elapsed_ms > 0
        res2, x2 = d.cg(rhs, tolerance=tol, engine=0)
        assert (res2.iterations, res2.relative_residual) == (res.iterations, res.relative_residual)
        ic.assert_bits(x2, x, name)
        d.close()


@pytest.mark.parametrize("b", (2, 3, 4))
def test_at_most_half_the_steps_of_block_jacobi(gpu, b):
    n, brp, bc, bv = ic.laplacian_system(16, b)
    rhs = np.random.default_rng(11).uniform(-1.0, 1.0, n).astype(np.float32)
    d = Dev(gpu, n, b, brp, bc, bv)
    d.factor()
    res, _ = d.cg(rhs, tolerance=TOL, engine=0)
    d.d_x.copyFromHost(np.zeros(n, np.float32), n)
    jac = gpu.cg_solve_bsr(d.A, d.d_b, d.d_x, gpu.CGConfig(tolerance=TOL, engine=0, preconditioner=2))
    print("b", b, "block IC(0)", res.iterations, "BLOCK_JACOBI", jac.iterations)
    assert res.error_code == 0 and res.converged and jac.error_code == 0 and jac.converged
    assert 2 * res.iterations <= jac.iterations, (b, res.iterations, jac.iterations)
    d.close()


def test_the_rules_of_cg_h(gpu):
    b = 3
    name, n, brp, bc, bv, rhs, tol = ic.parity_systems(b)[0]
    d = Dev(gpu, n, b, brp, bc, bv)
    d.factor()
    full, x_full = d.cg(rhs, tolerance=tol, engine=0)
    assert full.converged and full.iterations >= 3
    x0 = np.full(n, 0.5, np.float32)
    res, x = d.cg(rhs, x0=x0, tolerance=tol, max_iterations=0)
    assert (res.error_code, res.iterations, res.converged) == (0, 0, 0) and np.array_equal(x, x0)
    res, _ = d.cg(rhs, tolerance=tol, max_iterations=2)
    assert (res.error_code, res.iterations, res.converged, res.breakdown) == (0, 2, 0, 0)
    res, x = d.cg(rhs, tolerance=tol, max_iterations=full.iterations + 5)
    assert res.iterations == full.iterations
    ic.assert_bits(x, x_full, "steps after done change nothing")
    res, x = d.cg(np.zeros(n, np.float32), x0=x0, tolerance=tol)                # b = 0
    assert (res.error_code, res.converged, res.iterations, res.breakdown) == (0, 1, 0, 0) and not x.any()
    res, x = d.cg(rhs, x0=x_full, tolerance=1e-3)                               # a converged guess
    assert (res.error_code, res.converged, res.iterations) == (0, 1, 0)
    ic.assert_bits(x, x_full, "a converged guess is left alone")
    d.close()
    # an indefinite A breaks down at the last good iterate: p.q <= 0 at the first step
    d = Dev(gpu, n, b, brp, bc, -bv)
    pos = Dev(gpu, n, b, brp, bc, bv)
    pos.factor()
    d.gpu.bsr_destroy(d.F)
    c = d.A.contents
    d.F = gpu.bsr_wrap_device(n, n, b, c.num_blocks, addr(c.d_block_row_ptrs), addr(c.d_block_cols), pos.d_f.get())
    res, x = d.cg(rhs, x0=x0, tolerance=tol, engine=0)
    assert (res.error_code, res.converged, res.breakdown) == (0, 0, 1)
    ic.assert_bits(x, x0, "x stays at the last good iterate")
    d.close()
    pos.close()


def test_a_refilled_matrix_with_a_refactored_factor_is_not_stale(gpu):
    b = 2
    name, n, brp, bc, bv, rhs, tol = ic.parity_systems(b)[0]
    d = Dev(gpu, n, b, brp, bc, bv)
    d.factor()
    first, x1 = d.cg(rhs, tolerance=tol, engine=0)
    scaled = (bv * np.float32(4.0)).astype(np.float32)                      # the same pattern, new values
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(addr(d.A.contents.d_values)), gpu._np_ptr(scaled),
                                       scaled.nbytes) == 0
    gpu.bsr_invalidate_gpu_cache(d.A)
    res = gpu.bsr_ic0(d.A, d.d_f)
    assert res.error_code == 0 and res.analysis_ms > 0
    H = gpu.bsr_from_arrays(n, n, b, brp, bc, scaled)
    ic.assert_bits(d.d_f.copyToHost(d.count), gpu.bsr_ic0_cpu(H)[0], "refactored")
    gpu.bsr_destroy(H)
    second, x2 = d.cg(rhs, tolerance=tol, engine=0)
    assert second.error_code == 0 and second.converged and second.iterations == first.iterations
    assert np.allclose(x2 * 4.0, x1, rtol=1e-4, atol=1e-6)
    d.close()


@pytest.mark.parametrize("case", ("negative", "nan", "inf", "missing"))
def test_a_bad_factor_diagonal_is_rejected_on_the_device_and_x_is_untouched(gpu, case):
    b = 2
    name, n, brp, bc, bv, rhs, tol = ic.parity_systems(b)[0]
    d = Dev(gpu, n, b, brp, bc, bv)
    _, f = d.factor()
    x0 = np.full(n, 0.25, np.float32)
    if case == "missing":
        keep = np.ones(bc.size, bool)
        keep[ic.diagonal_positions(brp, bc)[5]] = False
        brp_m = brp.copy()
        brp_m[6:] -= 1
        other = Dev(gpu, n, b, brp_m, bc[keep], f.reshape(-1, b, b)[keep].reshape(-1))
        F = other.A
    else:
        bad = f.reshape(-1, b, b).copy()
        bad[ic.diagonal_positions(brp, bc)[5], 1, 1] = {"negative": -1.0, "nan": np.nan, "inf": np.inf}[case]
        d.d_f.copyFromHost(bad.reshape(-1), d.count)
        F = d.F
    d.d_b.copyFromHost(rhs, n)
    d.d_x.copyFromHost(x0, n)
    res = gpu.cg_solve_bsr_ic(d.A, F, d.d_b, d.d_x, gpu.CGConfig(tolerance=tol, engine=0))
    assert res.error_code == ARGUMENT, (case, res.error_code)
    ic.assert_bits(d.d_x.copyToHost(n), x0, case)
    if case == "missing":
        other.close()
    # a malformed factor pattern: INVALID_FORMAT before anything is written
    bad_col = bc.copy()
    bad_col[1] = len(brp) - 1
    other = Dev(gpu, n, b, brp, bad_col, bv)
    res = gpu.cg_solve_bsr_ic(d.A, other.A, d.d_b, d.d_x, gpu.CGConfig(tolerance=tol, engine=0))
    assert res.error_code == FORMAT
    ic.assert_bits(d.d_x.copyToHost(n), x0, case)
    other.close()
    d.close()


def test_cpp_bsr_ic_smoke(gpu):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "bsr_ic_smoke")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
