"""Reverse Cuthill-McKee (include/spmv/reorder.h) on the device.

csr_rcm against csr_rcm_cpu, int for int in d_perm and d_inverse, with equal components and levels: every graph of the
host test, and the edges where the kernels can go wrong: level widths around the one-workgroup limit of 256 with a hub
row that owns a whole level, a thousand levels of width one (the run kernel's level limit and several host batches),
wide levels whose parents own three children each (the scan across workgroups), parents with 63, 64, 65 and 130
children (the in-row prefix carry), the wide levels of a 2-D grid, a level past the grid cap, every lane count, both
values of peripheral and symmetric_pattern with a broken promise, 7, 8 and 9 components, views into poisoned buffers,
two runs and a second stream, every rejection with the outputs still poisoned.  csr_band_gpu against csr_band_cpu.
And the pipeline the feature exists for: rcm_reorder -> permute_gather -> spmv_csr / cg_solve / ic0_csr / sptrsv_csr ->
permute_gather.

The reference of every ordering is computed once per graph and config (the module-level cache) and never changed."""
import importlib
import json
import os

import numpy as np
import pytest

import array_views
import exact_data as ed
import rcm_cases as cases
import reorder_cases as rc
from conftest import ROOT
from test_gpu_bicgstab import bits, true_residual

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
POISON = np.int32(-77)
TOL = 1e-6
LANES = (1, 2, 4, 8, 16, 32, 64)
NARROW = 256                     # kNarrow (csrc/rcm_impl.h): the widest level the one-workgroup run kernel numbers
RUN_LEVELS = 512                 # kRunLevels: levels per launch of it
GRID_CAP = 2048                  # kMaxResidentBlocks: workgroups of the wide kernels, 256 / lanes rows each


# ------------------------------------------------------------------------------------------ helpers
def on_device(gpu, rows, cols, rp, ci, va):
    A = gpu.csr_from_arrays(rows, cols, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    return A


def int_buffer(gpu, values):
    values = np.ascontiguousarray(values, np.int32)
    buf = gpu.CudaBuffer(max(values.size, 1), "int32")
    if values.size:
        buf.copyFromHost(values, values.size)
    return buf


def float_buffer(gpu, values):
    values = np.ascontiguousarray(values, np.float32).reshape(-1)
    buf = gpu.CudaBuffer(max(values.size, 1))
    if values.size:
        buf.copyFromHost(values, values.size)
    return buf


class Graph:
    """a square matrix on the device with the host orderings it is compared against, computed once per config"""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = on_device(gpu, n, n, rp, ci, va)
        self.d_perm, self.d_inverse = int_buffer(gpu, np.full(n, POISON)), int_buffer(gpu, np.full(n, POISON))
        self.expected = {}

    def want(self, peripheral=1, promised=0):
        key = (peripheral, promised)
        if key not in self.expected:
            status, perm, inverse, components, levels = self.gpu.csr_rcm_cpu(
                self.A, self.gpu.RcmConfig(symmetric_pattern=promised, peripheral=peripheral))
            assert status == 0
            perm.setflags(write=False)
            inverse.setflags(write=False)
            self.expected[key] = (perm, inverse, components, levels)
        return self.expected[key]

    def check(self, peripheral=1, promised=0, lanes=0, what=""):
        gpu, n = self.gpu, self.n
        perm, inverse, components, levels = self.want(peripheral, promised)
        self.d_perm.copyFromHost(np.full(n, POISON), n)
        self.d_inverse.copyFromHost(np.full(n, POISON), n)
        res = gpu.csr_rcm(self.A, self.d_perm, self.d_inverse,
                          gpu.RcmConfig(symmetric_pattern=promised, peripheral=peripheral, lanes_per_row=lanes))
        assert res.error_code == 0, (what, gpu.spmv_error_string(res.error_code))
        got_perm, got_inverse = self.d_perm.copyToHost(n), self.d_inverse.copyToHost(n)
        tag = (what, peripheral, promised, lanes)
        assert np.array_equal(got_perm, perm), (tag, np.flatnonzero(got_perm != perm)[:8])
        assert np.array_equal(got_inverse, inverse), (tag, np.flatnonzero(got_inverse != inverse)[:8])
        assert (res.components, res.levels) == (components, levels), (tag, res.components, res.levels)
        assert res.launches >= 2 and res.elapsed_ms > 0 and res.sweeps >= 0
        return res

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.d_perm.release()
        self.d_inverse.release()


def prefix_carry_graph():
    """parents with 63, 64, 65 and 130 children: below, at and past one and two steps of a 64-lane row walk"""
    return cases.shuffle(cases.fans([63, 64, 65, 130]), 3)


GPU_CASES = {name: make for name, make in cases.CASES.items()}
GPU_CASES.update({
    "star(255)": lambda: cases.star(255), "star(256)": lambda: cases.star(256), "star(257)": lambda: cases.star(257),
    "star(5000)": lambda: cases.star(5000),
    "path(1000)": lambda: rc.tridiagonal(1000),
    "shuffled tree(3, 8)": lambda: cases.shuffle(cases.tree(3, 8), 1),
    "prefix carry": prefix_carry_graph,
    "7 3-paths": lambda: cases.disjoint_paths(7), "8 3-paths": lambda: cases.disjoint_paths(8),
    "9 3-paths": lambda: cases.disjoint_paths(9),
    "upper_bidiagonal(300)": lambda: rc.upper_bidiagonal(300),
})

_graphs = {}


@pytest.fixture(scope="module")
def graphs(gpu):
    def get(name):
        if name not in _graphs:
            _graphs[name] = Graph(gpu, *GPU_CASES[name]())
        return _graphs[name]
    yield get
    for g in _graphs.values():
        g.close()
    _graphs.clear()


# ------------------------------------------------------------------------------------------ csr_rcm
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_rcm_equals_the_host_ordering(gpu, graphs, name):
    g = graphs(name)
    res = g.check(what=name)
    print(name, "components", res.components, "levels", res.levels, "sweeps", res.sweeps, "launches", res.launches)


@pytest.mark.parametrize("name", ["block_mix", "K5", "upper_bidiagonal(9)", "upper_bidiagonal(300)", "shuffled poisson2d(24)",
                                  "shuffled convdiff2d(16)", "shuffled random_nonsym(300, 5, 1)", "star(257)",
                                  "9 3-paths"])
def test_config_corners(gpu, graphs, name):
    """no search; only A's rows walked, which for the bidiagonal and the non-symmetric matrices is the broken promise"""
    g = graphs(name)
    for peripheral in (0, 1):
        for promised in (0, 1):
            g.check(peripheral=peripheral, promised=promised, what=name)


def test_known_shapes(gpu, graphs):
    # a star from a leaf: leaf, hub, the other leaves; the widest level is leaves - 1 wide: 254, 255, 256 and 4999
    for leaves in (255, 256, 257, 5000):
        perm, inverse, components, levels = graphs("star(%d)" % leaves).want()
        assert (components, levels) == (1, 3)
        assert inverse[0] == leaves - 1                              # the hub is second in the sequence
    assert graphs("path(1000)").want()[2:] == (1, 1000) and 1000 > RUN_LEVELS
    assert graphs("64 3-paths").want()[2:] == (64, 192)
    perm, inverse, components, levels = graphs("shuffled tree(3, 8)").want()
    assert (components, levels) == (1, 17)                           # leaf to leaf through the root
    g = graphs("upper_bidiagonal(300)")
    assert g.want(1, 0)[2:] == (1, 300) and g.want(1, 1)[2] > 1
    assert not np.array_equal(g.want(1, 0)[0], g.want(1, 1)[0])


@pytest.mark.parametrize("name", ["shuffled poisson3d(8)", "star(5000)", "prefix carry"])
def test_every_lane_count(gpu, graphs, name):
    for lanes in LANES:
        graphs(name).check(lanes=lanes, what=(name, lanes))
    graphs(name).check(lanes=64, peripheral=0, what=name)


def test_wide_levels_on_a_grid(gpu):
    """shuffled poisson2d(300): the anti-diagonals grow to 300 vertices, past the one-workgroup limit and back"""
    g = Graph(gpu, *cases.shuffle(spd.poisson2d(300), 1))
    res = g.check(what="poisson2d(300)")
    assert (res.components, res.levels) == (1, 599) and 300 > NARROW
    status, lower, upper, profile = gpu.csr_band_cpu(g.A)
    B = gpu.csr_create(0, 0, 0)
    assert gpu.csr_permute_cpu(B, g.A, *g.want()[:2]) == 0
    after = gpu.csr_band_cpu(B)
    print("poisson2d(300) shuffled: band", (lower, upper, profile), "->", after[1:], "sweeps", res.sweeps,
          "launches", res.launches, "ms", res.elapsed_ms)
    assert after[1] == after[2] == 300
    g.check(lanes=1, what="poisson2d(300)")
    gpu.csr_destroy(B)
    g.close()


def test_a_level_past_the_grid_cap(gpu):
    """a tree of two levels of 725 children: from a leaf, the level of the other hubs' leaves is 724 * 725 = 524 900
    vertices wide, past 2048 workgroups of 256 rows at one lane per row; 725 parents own 725 children each"""
    arity = 725
    assert (arity - 1) * arity > GRID_CAP * 256
    g = Graph(gpu, *cases.tree(arity, 2))
    res = g.check(lanes=1, what="tree(725, 2)")
    assert (res.components, res.levels) == (1, 5)
    g.close()


def test_views_into_poisoned_buffers(gpu, graphs):
    g = graphs("shuffled poisson3d(8)")
    perm, inverse, components, levels = g.want()
    for offsets in ((1, 2, 3), (3, 1, 2)):
        with array_views.Views(gpu) as views:
            A, _ = views.csr(g.n, g.n, g.rp, g.ci, g.va, offsets)
            v_perm, v_inverse = views.out(g.n, offsets[0]), views.out(g.n, offsets[1])
            res = gpu.csr_rcm(A, v_perm.ptr, v_inverse.ptr)
            assert res.error_code == 0 and (res.components, res.levels) == (components, levels)
            assert np.array_equal(v_perm.download().view(np.int32), perm)
            assert np.array_equal(v_inverse.download().view(np.int32), inverse)
            assert gpu.csr_band_gpu(A) == gpu.csr_band_cpu(g.A)
            views.check_guards("csr_rcm")


def test_two_runs_and_a_second_stream_give_the_same_ints(gpu, graphs):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        for name in ("shuffled random_spd(500, 7, 3)", "shuffled tree(3, 8)"):
            g = graphs(name)
            first = g.check(what=name)
            second = g.check(what=name)
            assert (first.sweeps, first.launches) == (second.sweeps, second.launches)
            for st in streams:
                gpu.set_stream(st.cuda_stream)
                other = g.check(what=(name, "stream"))
                g.check(lanes=8, peripheral=0, what=(name, "stream"))
                assert (other.sweeps, other.launches) == (first.sweeps, first.launches)
    finally:
        gpu.set_stream(None)


def test_rejections_leave_the_outputs_untouched(gpu, graphs):
    E = gpu.SpMVError
    Cfg = gpu.RcmConfig
    g = graphs("path(10)")
    n = g.n
    p, q = int_buffer(gpu, np.full(n, POISON)), int_buffer(gpu, np.full(n, POISON))
    R = on_device(gpu, 3, 4, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 3], np.int32), np.ones(3, np.float32))
    assert gpu.csr_rcm(R, p, q).error_code == E.INVALID_DIMENSION
    H = gpu.csr_from_arrays(n, n, g.rp, g.ci, g.va)
    assert gpu.csr_rcm(H, p, q).error_code == E.INVALID_FORMAT                   # no device arrays
    for cfg in (Cfg(lanes_per_row=3), Cfg(lanes_per_row=128), Cfg(lanes_per_row=-1), Cfg(peripheral=2),
                Cfg(peripheral=-1), Cfg(reserved=1)):
        assert gpu.csr_rcm(g.A, p, q, cfg).error_code == E.INVALID_ARGUMENT
    # the device passes: the structure, then the ascent
    bad_col, bad_neg, bad_rp, bad_first = g.ci.copy(), g.ci.copy(), g.rp.copy(), g.rp.copy()
    bad_col[5], bad_neg[0], bad_rp[3], bad_first[0] = n, -1, g.rp[4] + 1, 1
    unsorted, repeated = g.ci.copy(), g.ci.copy()
    unsorted[[2, 3]] = unsorted[[3, 2]]                                          # row 1 is (0, 1, 2)
    repeated[3] = repeated[2]
    mn, mrp, mci, mva = rc.messy()
    broken = [(n, g.rp, bad_col, g.va), (n, g.rp, bad_neg, g.va), (n, bad_rp, g.ci, g.va), (n, bad_first, g.ci, g.va),
              (n, g.rp, unsorted, g.va), (n, g.rp, repeated, g.va), (mn, mrp, mci, mva)]
    broken += [make() for make in cases.RAW.values()]
    for rows, rp, ci, va in broken:
        M = on_device(gpu, rows, rows, rp, ci, va)
        pp, qq = int_buffer(gpu, np.full(rows, POISON)), int_buffer(gpu, np.full(rows, POISON))
        B = gpu.csr_create(0, 0, 0)
        for promised in (0, 1):
            assert gpu.csr_rcm(M, pp, qq, Cfg(symmetric_pattern=promised)).error_code == E.INVALID_FORMAT
            assert gpu.rcm_reorder(B, M, pp, qq, Cfg(symmetric_pattern=promised)).error_code == E.INVALID_FORMAT
        assert gpu.csr_rcm_cpu(M)[0] == E.INVALID_FORMAT
        assert np.all(pp.copyToHost(rows) == POISON) and np.all(qq.copyToHost(rows) == POISON)
        assert (B.contents.num_rows, B.contents.nnz) == (0, 0)
        gpu.csr_destroy(M)
        gpu.csr_destroy(B)
        pp.release()
        qq.release()
    short = gpu.csr_wrap_device(n, n, g.ci.size - 1, g.A.contents.d_row_ptrs, g.A.contents.d_col_indices,
                                g.A.contents.d_values)                           # row_ptrs[n] != nnz
    assert gpu.csr_rcm(short, p, q).error_code == E.INVALID_FORMAT
    assert gpu.csr_band_gpu(short)[0] == E.INVALID_FORMAT
    assert np.all(p.copyToHost(n) == POISON) and np.all(q.copyToHost(n) == POISON)
    Z = gpu.csr_create(0, 0, 0)
    res = gpu.csr_rcm(Z, p, q)
    assert (res.error_code, res.components, res.levels) == (0, 0, 0) and np.all(p.copyToHost(n) == POISON)
    for M in (R, H, short, Z):
        gpu.csr_destroy(M)
    p.release()
    q.release()


# ------------------------------------------------------------------------------------------ csr_band_gpu
BAND_CASES = {
    "rectangular": lambda: rc.with_row_lengths([3, 0, 17, 1, 64, 5, 65, 9, 0, 33] * 3 + [7] * 7, 91, seed=1),
    "wide": lambda: rc.with_row_lengths([5, 0, 0, 2], 600, seed=3),
    "tall": lambda: rc.with_row_lengths([2] * 3000, 7, seed=4),
    "long rows": lambda: rc.with_row_lengths([5000, 3, 0, 700], 6000, seed=3),
    "no entries": lambda: rc.with_row_lengths([0] * 9, 9, seed=5),
    "one entry last": lambda: rc.with_row_lengths([0] * 700 + [1], 5, seed=6),
}


@pytest.mark.parametrize("name", list(BAND_CASES))
def test_band_equals_the_host(gpu, name):
    rows, cols, rp, ci, va = BAND_CASES[name]()
    A = on_device(gpu, rows, cols, rp, ci, va)
    got = gpu.csr_band_gpu(A)
    assert got == gpu.csr_band_cpu(A) == (0,) + cases.band(rows, rp, ci), name
    gpu.csr_destroy(A)


def test_band_of_the_graphs_and_past_the_grid_cap(gpu, graphs):
    for name in ("shuffled poisson2d(24)", "star(5000)", "diagonal_only(7)", "upper_bidiagonal(300)", "messy"):
        n, rp, ci, va = (GPU_CASES[name] if name in GPU_CASES else rc.SMALL[name])()
        A = on_device(gpu, n, n, rp, ci, va)
        assert gpu.csr_band_gpu(A) == gpu.csr_band_cpu(A) == (0,) + cases.band(n, rp, ci), name
        gpu.csr_destroy(A)
    n, rp, ci, va = rc.tridiagonal(GRID_CAP * 64 + 37)               # mean row length 3: four lanes a row
    A = on_device(gpu, n, n, rp, ci, va)
    assert gpu.csr_band_gpu(A) == (0, 1, 1, n - 1)
    gpu.csr_destroy(A)
    Z = gpu.csr_create(0, 0, 0)
    assert gpu.csr_band_gpu(Z) == (0, 0, 0, 0)
    gpu.csr_destroy(Z)


# ------------------------------------------------------------------------------------------ the pipeline
class Reordered:
    """rcm_reorder of a matrix: B = P A P^T on the device, the two index arrays on both sides"""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, va
        self.A = on_device(gpu, n, n, rp, ci, va)
        self.B = gpu.csr_create(0, 0, 0)
        self.d_perm, self.d_inverse = int_buffer(gpu, np.full(n, POISON)), int_buffer(gpu, np.full(n, POISON))
        self.res = gpu.rcm_reorder(self.B, self.A, self.d_perm, self.d_inverse)
        assert self.res.error_code == 0, gpu.spmv_error_string(self.res.error_code)
        self.perm, self.inverse = self.d_perm.copyToHost(n), self.d_inverse.copyToHost(n)
        status, perm, inverse, components, levels = gpu.csr_rcm_cpu(self.A)
        assert status == 0 and np.array_equal(self.perm, perm) and np.array_equal(self.inverse, inverse)
        assert (self.res.components, self.res.levels) == (components, levels)
        # B is csr_permute_cpu's, byte for byte
        C = gpu.csr_create(0, 0, 0)
        assert gpu.csr_permute_cpu(C, self.A, perm, inverse) == 0 and gpu.csr_from_gpu(self.B) == 0
        for got, want in zip(gpu.csr_host_arrays(self.B), gpu.csr_host_arrays(C)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        gpu.csr_destroy(C)
        self.buffers = [self.d_perm, self.d_inverse]

    def buffer(self, values):
        self.buffers.append(float_buffer(self.gpu, values))
        return self.buffers[-1]

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.gpu.csr_destroy(self.B)
        for b in self.buffers:
            b.release()


def test_pipeline_spmv_is_bit_exact_on_exact_data(gpu):
    """integer values and an integer x: every row sum is exact in any order, so y = P^T (B (P x)) is A x bit for bit"""
    n, rp, ci, va = cases.shuffle(rc.coalesced(*ed.integer_spd(1500, 4000, 5)), 2)
    x = np.random.default_rng(6).integers(-64, 65, n).astype(np.float32)
    ed.check_exact(rp, ci, va, x)
    r = Reordered(gpu, n, rp, ci, va)
    d_x, d_px, d_py, d_y, d_ref = (r.buffer(x), r.buffer(np.zeros(n)), r.buffer(np.zeros(n)), r.buffer(np.zeros(n)),
                                   r.buffer(np.zeros(n)))
    for kernel in (0, 1, 2):
        cfg = gpu.SpMVConfig(kernel_type=kernel)
        assert gpu.spmv_csr(r.A, d_x, d_ref, cfg, n).error_code == 0
        assert gpu.permute_gather(d_px, d_x, r.d_perm, n) == 0
        assert gpu.spmv_csr(r.B, d_px, d_py, cfg, n).error_code == 0
        assert gpu.permute_gather(d_y, d_py, r.d_inverse, n) == 0
        y, ref = d_y.copyToHost(n), d_ref.copyToHost(n)
        assert np.array_equal(bits(ref), bits(ed.exact_reference(rp, ci, va, x)))
        assert np.array_equal(bits(y), bits(ref)), kernel
    before, after = gpu.csr_band_gpu(r.A), gpu.csr_band_gpu(r.B)
    assert after == gpu.csr_band_cpu(r.B) and after[0] == 0
    print("integer_spd(1500): band", before[1:], "->", after[1:])
    r.close()


@pytest.mark.parametrize("name", ["shuffled poisson2d(24)", "shuffled poisson3d(8)", "shuffled poisson2d(64)"])
def test_pipeline_band_cg_ic0_and_sptrsv(gpu, name):
    with open(os.path.join(ROOT, "tests", "golden", cases.GOLDEN)) as f:
        recorded = json.load(f)[name]
    n, rp, ci, va = cases.RECORDED[name]()
    r = Reordered(gpu, n, rp, ci, va)
    assert list(gpu.csr_band_gpu(r.A)[1:]) == recorded["before"]
    assert list(gpu.csr_band_gpu(r.B)[1:]) == recorded["after"]
    assert (r.res.components, r.res.levels) == (recorded["components"], recorded["levels"])
    if name in cases.QUOTED:
        assert max(gpu.csr_band_gpu(r.B)[1:3]) == cases.QUOTED[name][1]

    # cg_solve in the new numbering, the answer in the old; the reference is the same solver on A itself, and the
    # bound is test_gpu_cg.py's: the recurrence stops at TOL, the true fp64 residual of an fp32 solve may be 4 TOL,
    # or twice what the reference solve's is
    b = np.random.default_rng(1).uniform(-1.0, 1.0, n).astype(np.float32)
    d_b, d_pb, d_px, d_x, d_ref = (r.buffer(b), r.buffer(np.zeros(n)), r.buffer(np.zeros(n)), r.buffer(np.zeros(n)),
                                   r.buffer(np.zeros(n)))
    cfg = gpu.CGConfig(tolerance=TOL, engine=0, preconditioner=1)
    ref = gpu.cg_solve(r.A, d_b, d_ref, cfg)
    assert ref.error_code == 0 and ref.converged == 1
    assert gpu.permute_gather(d_pb, d_b, r.d_perm, n) == 0
    res = gpu.cg_solve(r.B, d_pb, d_px, cfg)
    assert res.error_code == 0 and res.converged == 1
    assert gpu.permute_gather(d_x, d_px, r.d_inverse, n) == 0
    true = true_residual(rp, ci, va, b, d_x.copyToHost(n))
    bound = max(4 * TOL, 2 * true_residual(rp, ci, va, b, d_ref.copyToHost(n)))
    print(f"{name}: CG {res.iterations} steps on B, {ref.iterations} on A; true residual {true:.3e} bound {bound:.3e}")
    assert true <= bound, (name, true, bound)

    # ic0_csr and sptrsv_csr take B: the factor is the host's bit for bit, both triangles solve, and IC-preconditioned
    # CG needs fewer steps than Jacobi's
    nnz = r.B.contents.nnz
    d_factor = gpu.CudaBuffer(nnz)
    r.buffers.append(d_factor)
    fact = gpu.ic0_csr(r.B, d_factor)
    assert fact.error_code == 0 and fact.bad_pivot == -1
    l_host, bad = gpu.ic0_cpu_csr(r.B)
    assert bad == -1 and np.array_equal(bits(d_factor.copyToHost(nnz)), bits(l_host))
    m = r.B.contents
    F = gpu.csr_wrap_device(n, n, nnz, m.d_row_ptrs, m.d_col_indices, d_factor.get())
    d_t = r.buffer(np.zeros(n))
    for uplo, src in ((0, d_pb), (1, d_t)):
        solve = gpu.sptrsv_csr(F, src, d_t, gpu.SpTRSVConfig(uplo=uplo, diag=0))
        assert solve.error_code == 0 and solve.num_levels >= 1
    d_px.copyFromHost(np.zeros(n, np.float32), n)
    res_ic = gpu.cg_solve_ic(r.B, F, d_pb, d_px, gpu.CGConfig(tolerance=TOL, engine=0))
    assert res_ic.error_code == 0 and res_ic.converged == 1 and res_ic.iterations < res.iterations
    gpu.csr_destroy(F)
    r.close()
