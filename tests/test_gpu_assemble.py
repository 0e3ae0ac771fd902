"""Matrix assembly (include/spmv/assemble.h) on the device.

csr_from_coo_gpu against csr_from_coo_cpu and against the restatement of tests/assemble_cases.py: row_ptrs, col_indices
and the bit patterns of the values at zero tolerance, in both modes, on every case: the tile edges of the sort (sizes
taken from result.tile_entries), the key widths with the pass counts they must give, sorted / reversed / shuffled input,
duplicate runs across a workgroup edge and across a wavefront edge, the degenerate shapes, and the values whose sum
depends on the order or whose bits are easy to lose.  csr_coo_refill (and its async form) against a fresh assembly, with
the cached tiled plan it must drop.  Views into larger buffers with guard words.  The rejections.  Two streams.
csr_row_indices_gpu and the round trip.  A Q1 grid assembled on the device and solved, refilled and solved again.  The
C++ caller.

The references of a case are computed once (the module-level cache below) and never changed."""
import os
import subprocess

import numpy as np
import pytest

import array_views
import assemble_cases as ac
from conftest import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = array_views.SENTINEL


# ------------------------------------------------------------------------------------------ helpers
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


def download(gpu, C):
    assert gpu.csr_from_gpu(C) == 0
    return gpu.csr_host_arrays(C)


def tile_entries(gpu):
    return gpu.csr_from_coo_gpu(None, 1, 1, 0, None, None, None).tile_entries


class Triplets:
    """one case on the device, with its references per mode"""

    def __init__(self, gpu, case):
        self.gpu = gpu
        self.num_rows, self.num_cols, self.rows, self.cols, self.vals = case
        self.n = len(self.rows)
        self.d_rows, self.d_cols = int_buffer(gpu, self.rows), int_buffer(gpu, self.cols)
        self.d_vals = float_buffer(gpu, self.vals)
        self.expected = {}

    def want(self, mode, vals=None):
        key = (mode, None if vals is None else vals.tobytes())
        if key not in self.expected:
            v = self.vals if vals is None else vals
            C = self.gpu.csr_create(0, 0, 0)
            assert self.gpu.csr_from_coo_cpu(C, self.num_rows, self.num_cols, self.rows, self.cols, v,
                                             self.gpu.CooConfig(duplicates=mode)) == 0
            host = self.gpu.csr_host_arrays(C)
            self.gpu.csr_destroy(C)
            restated = ac.assemble(self.num_rows, self.num_cols, self.rows, self.cols, v, mode)
            assert ac.same(host, restated)
            for a in host:
                a.setflags(write=False)
            self.expected[key] = host
        return self.expected[key]

    def build(self, mode, want_plan=False, d_vals=None):
        gpu = self.gpu
        C = gpu.csr_create(3, 3, 2)
        out = gpu.csr_from_coo_gpu(C, self.num_rows, self.num_cols, self.n, self.d_rows, self.d_cols,
                                   self.d_vals if d_vals is None else d_vals, gpu.CooConfig(duplicates=mode),
                                   want_plan=want_plan)
        res = out[0] if want_plan else out
        assert res.error_code == 0, gpu.spmv_error_string(res.error_code)
        return (C,) + (out if want_plan else (out,))

    def check(self, mode, what=""):
        gpu = self.gpu
        want = self.want(mode)
        C, res = self.build(mode)
        m = C.contents
        assert (m.num_rows, m.num_cols, m.nnz) == (self.num_rows, self.num_cols, want[1].size), what
        assert m.owns_device_memory and m.owns_host_memory
        got = download(gpu, C)
        gpu.csr_destroy(C)
        assert np.array_equal(got[0], want[0]), (what, mode, "row_ptrs")
        assert np.array_equal(got[1], want[1]), (what, mode, "col_indices", np.flatnonzero(got[1] != want[1])[:8])
        bad = np.flatnonzero(ac.bits(got[2]) != ac.bits(want[2]))
        assert bad.size == 0, (what, mode, "values", bad[:8], ac.bits(got[2])[bad[:8]], ac.bits(want[2])[bad[:8]])
        assert res.nnz_out == want[1].size and res.combined == self.n - want[1].size
        assert res.passes == ac.expected_passes(self.num_rows, self.num_cols, self.rows, self.cols), what
        assert res.tile_entries == tile_entries(gpu) and (res.launches > 0) == (self.n > 0)
        return res

    def close(self):
        for b in (self.d_rows, self.d_cols, self.d_vals):
            b.release()


CASE_NAMES = list(ac.cases(4096))          # the names do not depend on the tile, only the sizes behind them
_triplets = {}


@pytest.fixture(scope="module")
def triplets(gpu):
    made = ac.cases(tile_entries(gpu))

    def get(name):
        if name not in _triplets:
            _triplets[name] = Triplets(gpu, made[name]())
        return _triplets[name]
    yield get
    for t in _triplets.values():
        t.close()
    _triplets.clear()


# ------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_device_assembles_the_hosts_bits(gpu, triplets, name):
    t = triplets(name)
    for mode in ac.MODES:
        t.check(mode, name)


def test_pass_counts_of_the_key_widths(gpu, triplets):
    T = tile_entries(gpu)
    assert T % 64 == 0
    assert triplets("key 32 bits").check(ac.SUM).passes == 4          # a 32-bit key exactly: every digit differs
    assert triplets("key 33 bits").check(ac.SUM).passes == 5
    assert triplets("key 48 bits").check(ac.SUM).passes == 6
    assert triplets("top digit only").check(ac.SUM).passes == 1
    t = triplets("all equal")
    assert t.n == 17 * T + 3
    res = t.check(ac.SUM)
    assert (res.passes, res.nnz_out, res.combined) == (0, 1, t.n - 1)  # one segment of length n
    res = t.check(ac.KEEP)
    assert (res.passes, res.nnz_out, res.combined) == (0, t.n, 0)
    assert triplets("n=17T+3").check(ac.SUM).passes == 3   # 10 + 10 bits; 18 tiles: a second scan level


def test_the_runs_sit_where_their_names_say(gpu, triplets):
    """in sorted order the run of three equal keys begins at slot T - 1 (the last of a workgroup's tile and of the
    compress step's block) and at slot 63 (the last lane of a wavefront)"""
    T = tile_entries(gpu)
    for name, slot in (("run from slot T-1 to T+1", T - 1), ("run from slot 63", 63)):
        t = triplets(name)
        keep = t.want(ac.KEEP)
        assert np.array_equal(keep[1][slot - 1:slot + 4], [slot - 1, slot, slot, slot, slot + 1])
        res = t.check(ac.SUM, name)
        assert res.combined == 2


# ------------------------------------------------------------------------------------------ refill
def new_values(t, seed):
    """values of the same kinds in another arrangement: the case's own bit patterns, permuted"""
    return t.vals[np.random.default_rng(seed).permutation(t.n)].copy()


@pytest.mark.parametrize("name", ["n=1", "n=257", "three keys", "all equal", "1e8, 1, -1e8", "special values",
                                  "run from slot T-1 to T+1", "key 48 bits", "n=0"])
def test_refill_gives_the_bits_of_a_fresh_assembly(gpu, triplets, name):
    import torch
    t = triplets(name)
    side = torch.cuda.Stream()
    for mode in ac.MODES:
        C, res, plan = t.build(mode, want_plan=True)
        assert plan is not None
        assert gpu.coo_plan_info(plan) == (0, t.num_rows, t.num_cols, t.n, res.nnz_out, mode)
        before = download(gpu, C)
        for round_, sync in enumerate((True, False)):
            vals = new_values(t, 70 + round_)
            d_new = float_buffer(gpu, vals)
            if sync:
                assert gpu.csr_coo_refill(plan, C, d_new) == 0
            else:
                assert gpu.csr_coo_refill_async(plan, C, d_new, stream=side.cuda_stream) == 0
                side.synchronize()
            got = download(gpu, C)
            want = t.want(mode, vals)
            assert got[0].tobytes() == before[0].tobytes() and got[1].tobytes() == before[1].tobytes()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            assert np.array_equal(ac.bits(got[2]), ac.bits(want[2])), (name, mode, sync)
            # and a fresh device assembly of these values
            F, _ = t.build(mode, d_vals=d_new)
            assert ac.same(download(gpu, F), got)
            gpu.csr_destroy(F)
            d_new.release()
        gpu.coo_plan_destroy(plan)
        gpu.csr_destroy(C)


def test_refill_drops_the_cached_tiled_plan(gpu, triplets):
    """spmv_csr with use_texture caches a tiled copy of the values with the matrix; after csr_coo_refill the next call
    must multiply by the new ones"""
    old_debug = os.environ.get("SPMV_DEBUG")
    os.environ["SPMV_DEBUG"] = "min_cols=1,min_nnz=1"       # the tiled engine also for a matrix this small
    try:
        t = triplets("n=2T+1")
        C, res, plan = t.build(ac.SUM, want_plan=True)
        x = np.random.default_rng(5).standard_normal(t.num_cols).astype(np.float32)
        d_x, d_y = float_buffer(gpu, x), float_buffer(gpu, np.zeros(t.num_rows))
        tiled = gpu.SpMVConfig(kernel_type=gpu.SpMVConfig.VECTOR_CSR, use_texture=True)
        scalar = gpu.SpMVConfig(kernel_type=gpu.SpMVConfig.SCALAR_CSR)

        def products():
            assert gpu.spmv_csr(C, d_x, d_y, tiled, t.num_cols).error_code == 0
            y_tiled = d_y.copyToHost(t.num_rows)
            assert gpu.spmv_csr(C, d_x, d_y, scalar, t.num_cols).error_code == 0
            return y_tiled, d_y.copyToHost(t.num_rows)

        y_tiled, y_plain = products()
        assert gpu.csr_has_tiled_plan(C)
        assert np.allclose(y_tiled, y_plain, rtol=1e-4, atol=1e-3)
        vals = (new_values(t, 9) * np.float32(3.0) + np.float32(50.0)).astype(np.float32)
        d_new = float_buffer(gpu, vals)
        assert gpu.csr_coo_refill(plan, C, d_new) == 0
        assert not gpu.csr_has_tiled_plan(C)
        z_tiled, z_plain = products()
        assert not np.allclose(z_plain, y_plain, rtol=1e-4, atol=1e-3)           # the values did change
        assert np.allclose(z_tiled, z_plain, rtol=1e-4, atol=1e-3)               # and the tiled route sees them
        for b in (d_x, d_y, d_new):
            b.release()
        gpu.coo_plan_destroy(plan)
        gpu.csr_destroy(C)
    finally:
        if old_debug is None:
            os.environ.pop("SPMV_DEBUG", None)
        else:
            os.environ["SPMV_DEBUG"] = old_debug


def test_refill_rejections(gpu, triplets):
    E = gpu.SpMVError
    t = triplets("n=257")
    C, res, plan = t.build(ac.SUM, want_plan=True)
    before = download(gpu, C)
    for refill in (gpu.csr_coo_refill, gpu.csr_coo_refill_async):
        assert refill(None, C, t.d_vals) == E.INVALID_ARGUMENT
        assert refill(plan, None, t.d_vals) == E.INVALID_ARGUMENT
        assert refill(plan, C, None) == E.INVALID_ARGUMENT
        for shape in ((t.num_rows + 1, t.num_cols, res.nnz_out), (t.num_rows, t.num_cols - 1, res.nnz_out),
                      (t.num_rows, t.num_cols, res.nnz_out - 1)):
            W = gpu.csr_wrap_device(*shape, C.contents.d_row_ptrs, C.contents.d_col_indices, C.contents.d_values)
            assert refill(plan, W, t.d_vals) == E.INVALID_DIMENSION
            gpu.csr_destroy(W)
        H = gpu.csr_create(t.num_rows, t.num_cols, res.nnz_out)                 # the right size, host only
        assert refill(plan, H, t.d_vals) == E.INVALID_FORMAT
        gpu.csr_destroy(H)
    assert ac.same(download(gpu, C), before)
    gpu.coo_plan_destroy(plan)
    gpu.csr_destroy(C)


# ------------------------------------------------------------------------------------------ views, rejects, streams
@pytest.mark.parametrize("offsets", [(1, 2, 3), (3, 1, 0), (2, 3, 1)])
def test_inputs_that_are_views_into_larger_buffers(gpu, triplets, offsets):
    T = tile_entries(gpu)
    for name in ("n=T+1", "key 33 bits"):
        t = triplets(name)
        with array_views.Views(gpu) as views:
            v_rows = views.view(t.rows, offsets[0], np.int32(0))
            v_cols = views.view(t.cols, offsets[1], np.int32(0))
            v_vals = views.view(t.vals, offsets[2], np.float32(1234.5))
            for mode in ac.MODES:
                C = gpu.csr_create(0, 0, 0)
                res, plan = gpu.csr_from_coo_gpu(C, t.num_rows, t.num_cols, t.n, v_rows.ptr, v_cols.ptr, v_vals.ptr,
                                                 gpu.CooConfig(duplicates=mode), want_plan=True)
                assert res.error_code == 0
                assert ac.same(download(gpu, C), t.want(mode)), (name, mode, offsets)
                assert gpu.csr_coo_refill(plan, C, v_vals.ptr) == 0
                assert ac.same(download(gpu, C), t.want(mode)), (name, mode, offsets)
                views.check_guards((name, mode))
                gpu.coo_plan_destroy(plan)
                gpu.csr_destroy(C)
            for v, payload in ((v_rows, t.rows), (v_cols, t.cols), (v_vals, t.vals)):
                assert v.download().tobytes() == np.ascontiguousarray(payload).tobytes()      # only read


def test_guard_words_around_the_output_of_a_refill(gpu, triplets):
    """C's value array as a view with guard words: the refill writes nnz_out floats and nothing else"""
    t = triplets("n=257")
    want = t.want(ac.SUM)
    C, res, plan = t.build(ac.SUM, want_plan=True)
    with array_views.Views(gpu) as views:
        W, (v_rp, v_ci, v_va) = views.csr(t.num_rows, t.num_cols, want[0], want[1],
                                          np.full(want[1].size, SENTINEL, np.uint32).view(np.float32), (1, 2, 3))
        assert gpu.csr_coo_refill(plan, W, t.d_vals) == 0
        assert np.array_equal(ac.bits(v_va.download()), ac.bits(want[2]))
        assert np.array_equal(v_rp.download(), want[0]) and np.array_equal(v_ci.download(), want[1])
        views.check_guards("refill")
    gpu.coo_plan_destroy(plan)
    gpu.csr_destroy(C)


def test_rejects_leave_c_untouched(gpu):
    """an index out of range at the last position of the last tile: found by the device pass, before C is touched"""
    E = gpu.SpMVError
    T = tile_entries(gpu)
    num_rows, num_cols, rows, cols, vals = ac.uniform(40, 50, 3 * T, 8)
    d_cols, d_vals = int_buffer(gpu, cols), float_buffer(gpu, vals)
    C = gpu.csr_create(2, 3, 1)
    header = bytes(C.contents)
    for mode in ac.MODES:
        for array, bad in (("rows", num_rows), ("cols", -1), ("rows", -1), ("cols", num_cols)):
            r, c = rows.copy(), cols.copy()
            (r if array == "rows" else c)[-1] = bad
            d_r, d_c = int_buffer(gpu, r), int_buffer(gpu, c)
            res, plan = gpu.csr_from_coo_gpu(C, num_rows, num_cols, r.size, d_r, d_c, d_vals,
                                             gpu.CooConfig(duplicates=mode), want_plan=True)
            assert res.error_code == E.INVALID_FORMAT and plan is None, (array, bad)
            assert (res.nnz_out, res.combined, res.passes) == (0, 0, 0) and res.launches == 1
            assert bytes(C.contents) == header                    # the same pointers, sizes and flags: nothing adopted
            assert not C.contents.d_row_ptrs and not C.contents.d_values
            d_r.release()
            d_c.release()
    # a valid call afterwards still works into the same C
    d_rows = int_buffer(gpu, rows)
    assert gpu.csr_from_coo_gpu(C, num_rows, num_cols, rows.size, d_rows, d_cols, d_vals).error_code == 0
    assert ac.same(download(gpu, C), ac.assemble(num_rows, num_cols, rows, cols, vals))
    # no triplets: an all-zero row_ptrs, with and without rows
    for shape in ((5, 7), (0, 0), (0, 9)):
        res = gpu.csr_from_coo_gpu(C, shape[0], shape[1], 0, None, None, None)
        assert (res.error_code, res.nnz_out, res.passes) == (0, 0, 0)
        got = download(gpu, C)
        assert np.array_equal(got[0], np.zeros(shape[0] + 1)) and got[1].size == 0
        assert (C.contents.num_rows, C.contents.num_cols, C.contents.nnz) == (shape[0], shape[1], 0)
    gpu.csr_destroy(C)
    for b in (d_rows, d_cols, d_vals):
        b.release()


def test_two_builds_on_two_streams_give_the_same_bytes(gpu, triplets):
    import torch
    T = tile_entries(gpu)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        for name in ("n=17T+3", "1e8, 1, -1e8", "key 48 bits"):
            t = triplets(name)
            for mode in ac.MODES:
                results = []
                for st in streams:
                    gpu.set_stream(st.cuda_stream)
                    C, _ = t.build(mode)
                    results.append(b"".join(a.tobytes() for a in download(gpu, C)))
                    gpu.csr_destroy(C)
                assert results[0] == results[1]
                assert results[0] == b"".join(a.tobytes() for a in t.want(mode))
    finally:
        gpu.set_stream(None)


# ------------------------------------------------------------------------------------------ CSR -> COO -> CSR
def test_row_indices_and_the_round_trip(gpu):
    T = tile_entries(gpu)
    rng = np.random.default_rng(17)
    for rows, cols, n in ((1, 1, 1), (300, 200, 2 * T + 77), (5000, 3, 900), (3, 5000, T)):
        rp, ci, va = ac.assemble(*ac.uniform(rows, cols, n, 60 + rows))         # sorted, duplicate-free rows
        A = gpu.csr_from_arrays(rows, cols, rp, ci, va)
        assert gpu.csr_to_gpu(A) == 0
        nnz = ci.size
        d_rows = int_buffer(gpu, np.full(nnz, -9))
        assert gpu.csr_row_indices_gpu(A, d_rows) == 0
        row_of = d_rows.copyToHost(nnz)
        assert np.array_equal(row_of, np.repeat(np.arange(rows), np.diff(rp)))
        p = rng.permutation(nnz)
        d_r, d_c, d_v = int_buffer(gpu, row_of[p]), int_buffer(gpu, ci[p]), float_buffer(gpu, va[p])
        for mode in ac.MODES:
            C = gpu.csr_create(0, 0, 0)
            res = gpu.csr_from_coo_gpu(C, rows, cols, nnz, d_r, d_c, d_v, gpu.CooConfig(duplicates=mode))
            assert res.error_code == 0 and res.combined == 0
            assert ac.same(download(gpu, C), (rp, ci, va))
            gpu.csr_destroy(C)
        for b in (d_rows, d_r, d_c, d_v):
            b.release()
        gpu.csr_destroy(A)
    # a malformed matrix is rejected on the device before anything is written
    bad_rp = np.asarray([0, 3, 2, 4], np.int32)
    M = gpu.csr_from_arrays(3, 4, bad_rp, [0, 1, 2, 3], [1.0, 2.0, 3.0, 4.0])
    assert gpu.csr_to_gpu(M) == 0
    d_rows = int_buffer(gpu, np.full(4, -9))
    assert gpu.csr_row_indices_gpu(M, d_rows) == gpu.SpMVError.INVALID_FORMAT
    assert np.array_equal(d_rows.copyToHost(4), np.full(4, -9))
    d_rows.release()
    gpu.csr_destroy(M)


# ------------------------------------------------------------------------------------------ end to end
def solve(gpu, A, b, H=None):
    n = b.size
    d_b, d_x = float_buffer(gpu, b), float_buffer(gpu, np.zeros(n))
    cfg = gpu.CGConfig(tolerance=1e-6, max_iterations=500)
    res = gpu.cg_solve(A, d_b, d_x, cfg) if H is None else gpu.cg_solve_amg(A, H, d_b, d_x, cfg)
    assert res.error_code == 0 and res.converged
    x = d_x.copyToHost(n)
    d_b.release()
    d_x.release()
    return x, res.iterations


def test_a_q1_grid_assembled_on_the_device_and_solved(gpu):
    """33 x 33 nodes, 1024 elements, 16 contributions each: the device-assembled matrix is the host-assembled one bit
    for bit, so cg_solve gives the same bits in the same number of steps; after csr_coo_refill with scaled
    coefficients and amg_update, cg_solve_amg equals the same solve (the same set-up, the same update) on freshly
    assembled matrices"""
    n, rows, cols, vals = ac.q1_grid(33)
    assert rows.size == 16 * 32 * 32
    d_rows, d_cols, d_vals = int_buffer(gpu, rows), int_buffer(gpu, cols), float_buffer(gpu, vals)
    C = gpu.csr_create(0, 0, 0)
    res, plan = gpu.csr_from_coo_gpu(C, n, n, rows.size, d_rows, d_cols, d_vals, want_plan=True)
    assert res.error_code == 0 and res.nnz_out == (3 * 33 - 2) ** 2 and res.combined == rows.size - res.nnz_out
    H = gpu.csr_create(0, 0, 0)
    assert gpu.csr_from_coo_cpu(H, n, n, rows, cols, vals) == 0
    assert ac.same(download(gpu, C), gpu.csr_host_arrays(H))
    assert gpu.csr_to_gpu(H) == 0
    b = np.random.default_rng(2).standard_normal(n).astype(np.float32)
    x_dev, it_dev = solve(gpu, C, b)
    x_host, it_host = solve(gpu, H, b)
    assert it_dev == it_host and np.array_equal(ac.bits(x_dev), ac.bits(x_host))

    amg_res, hierarchy = gpu.amg_setup_device(C)
    assert amg_res.error_code == 0 and hierarchy is not None
    # the next step of a nonlinear solve: new coefficients, the same mesh
    scale = (1.0 + 3.0 * np.random.default_rng(3).random(32 * 32)).astype(np.float32)
    _, _, _, vals2 = ac.q1_grid(33, coefficient=scale)
    d_vals2 = float_buffer(gpu, vals2)
    assert gpu.csr_coo_refill(plan, C, d_vals2) == 0
    assert gpu.amg_update(hierarchy, C).error_code == 0
    x_refilled, it_refilled = solve(gpu, C, b, hierarchy)

    # the same solve without a refill: a hierarchy set up on a fresh assembly of the first values (amg_update keeps
    # the aggregates of the matrix it was set up on), updated with a fresh assembly of the second
    G, F = gpu.csr_create(0, 0, 0), gpu.csr_create(0, 0, 0)
    assert gpu.csr_from_coo_gpu(G, n, n, rows.size, d_rows, d_cols, d_vals).error_code == 0
    fresh_res, fresh = gpu.amg_setup_device(G)
    assert fresh_res.error_code == 0 and fresh_res.levels == amg_res.levels
    assert gpu.csr_from_coo_gpu(F, n, n, rows.size, d_rows, d_cols, d_vals2).error_code == 0
    assert ac.same(download(gpu, F), download(gpu, C))
    assert gpu.amg_update(fresh, F).error_code == 0
    x_fresh, it_fresh = solve(gpu, F, b, fresh)
    assert it_refilled == it_fresh and np.array_equal(ac.bits(x_refilled), ac.bits(x_fresh))

    gpu.amg_destroy(hierarchy)
    gpu.amg_destroy(fresh)
    gpu.coo_plan_destroy(plan)
    for M in (C, H, F, G):
        gpu.csr_destroy(M)
    for buf in (d_rows, d_cols, d_vals, d_vals2):
        buf.release()


def test_cpp_assemble_smoke(gpu, tmp_path):
    """tests/cpp/assemble_smoke.cpp through spmv/assemble.h and CudaBuffer, compiled here with build()'s g++ line."""
    exe = str(tmp_path / "assemble_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "assemble_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
