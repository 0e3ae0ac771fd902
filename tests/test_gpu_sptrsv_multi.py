"""sptrsv_csr_multi (include/spmv/sptrsv.h) on the device.

The contract is bitwise: column j of the batched solve is sptrsv_csr on that column alone at the same lanes_per_row.
So the reference in every comparison is sptrsv_csr itself (and sptrsv_cpu_csr where ordered = 1), at zero tolerance.
On top of that: integer systems proven exact in any summation order (tests/exact_triangles.py, the prover applied per
column) pin every column to the integer solution at every lane count; the layouts (leading dimensions, views 4 bytes
past a 16-byte boundary, poisoned padding, in place); independence of the columns; reproducibility across runs and
streams; the schedule shared with sptrsv_csr; the rejections with X untouched; and a C++ caller."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import exact_triangles
from array_views import SENTINEL, View
from conftest import ROOT
from test_gpu_sptrsv import EXACT_SPECS, LANES, NARROW

pytestmark = pytest.mark.gpu

POISON = SENTINEL.view(np.float32)
ALL_K = (1, 2, 3, 4, 5, 8, 9, 16, 32)
SOME_K = (3, 8, 9)
K_MAX = 32


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


@pytest.fixture(scope="module")
def nonsym():
    return importlib.import_module("gpu-spmv_amd.nonsym")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, tag=""):
    """bit for bit; a NaN must meet a NaN, whose sign and payload IEEE 754 leaves open (test_gpu_sptrsv.py)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(tag))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[keep], bits(want)[keep], err_msg=str(tag))


def set_lanes(monkeypatch, lanes):
    if lanes is None:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
    else:
        monkeypatch.setenv("SPMV_DEBUG", f"sptrsv_lanes={lanes}")


class Device:
    """A matrix on the device, sptrsv_csr on one column as the reference and sptrsv_csr_multi in any layout."""

    def __init__(self, gpu, n, rp, ci, va):
        self.gpu, self.n = gpu, n
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self.d_b, self.d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)

    def single(self, b, cfg):
        self.d_b.copyFromHost(np.ascontiguousarray(b, np.float32), self.n)
        res = self.gpu.sptrsv_csr(self.A, self.d_b, self.d_x, cfg)
        return res, self.d_x.copyToHost(self.n)

    def singles(self, B, cfg):
        """(result of column 0, X) of sptrsv_csr column by column"""
        out = [self.single(B[:, j], cfg) for j in range(B.shape[1])]
        assert all(r.error_code == 0 for r, _ in out)
        return out[0][0], np.stack([x for _, x in out], axis=1)

    def plain(self, B, cfg, in_place=False):
        """(result, X) of sptrsv_csr_multi on dense n x k buffers (ld = k)"""
        n, k = B.shape
        d_B = self.gpu.CudaBuffer(n * k)
        d_B.copyFromHost(np.ascontiguousarray(B, np.float32).ravel(), n * k)
        d_X = d_B if in_place else self.gpu.CudaBuffer(n * k)
        res = self.gpu.sptrsv_csr_multi(self.A, d_B, d_X, k, config=cfg)
        X = d_X.copyToHost(n * k).reshape(n, k)
        d_B.release()
        if not in_place:
            d_X.release()
        return res, X

    def multi(self, B, cfg, ldb=None, ldx=None, offset=0, in_place=False, x_fill=None):
        """(result, X) of sptrsv_csr_multi on the n x k array B stored with the given leading dimensions in views
        `offset` floats past a 16-byte boundary.  X's padding columns and both views' surroundings are poison: asserts
        that they, and B (unless the solve is in place), come back bit for bit.  The arrays end at the last row's
        column k."""
        n, k = B.shape
        ldb, ldx = ldb or k, ldx or k
        hb = np.full(n * ldb, POISON, np.float32)
        hb.reshape(n, ldb)[:, :k] = B
        hb = hb[:(n - 1) * ldb + k]
        vb = View(self.gpu, hb, offset, SENTINEL)
        if in_place:
            assert ldb == ldx
            vx, hx = vb, hb
        else:
            hx = np.full((n - 1) * ldx + k, POISON if x_fill is None else x_fill, np.float32)
            vx = View(self.gpu, hx, offset, SENTINEL)
        try:
            res = self.gpu.sptrsv_csr_multi(self.A, vb.ptr, vx.ptr, k, ldb, ldx, cfg)
            full = np.full(n * ldx, POISON, np.float32)
            full[:(n - 1) * ldx + k] = vx.download()
            got = full.reshape(n, ldx)
            vb.check_guards("B")
            vx.check_guards("X")
            if not in_place:
                assert np.array_equal(bits(vb.download()), bits(hb)), "B was written"
            want_pad = np.full(n * ldx, POISON, np.float32)
            want_pad[:hx.size] = hx
            assert np.array_equal(bits(got[:, k:]), bits(want_pad.reshape(n, ldx)[:, k:])), "X's padding was written"
            return res, got[:, :k].copy()
        finally:
            vb.release()
            if not in_place:
                vx.release()

    def close(self):
        self.gpu.csr_destroy(self.A)
        self.d_b.release()
        self.d_x.release()


def same_shape(res, ref, tag):
    assert res.error_code == 0, tag
    got = (res.num_levels, res.launches, res.lanes_per_row)
    assert got == (ref.num_levels, ref.launches, ref.lanes_per_row), (tag, got)


# ------------------------------------------------------------------------------------------ 1. exact data
def triangle_times(case, x):
    """T x in int64 (the triangle's off-diagonal entries and the diagonal, 1 with unit), as exact_triangles.make"""
    rows = np.repeat(np.arange(case.n), np.diff(case.rp))
    vals = case.va.astype(np.int64)
    inside = (case.ci < rows) if case.uplo == 0 else (case.ci > rows)
    on = case.ci == rows
    weight = np.where(inside, vals, np.where(on, 1 if case.unit else vals, 0))
    b = np.zeros(case.n, np.int64)
    np.add.at(b, rows, weight * x[case.ci])
    return b


_EXACT = {}


def exact_columns(index):
    """(case, B, X): the proven case of EXACT_SPECS[index] and as many integer columns as its test solves (32 for the
    two specs that run every k, 9 for the rest), column 0 the case's own, every
    other one drawn, multiplied out in integers and proven by exact_triangles.prove as a case of its own; a rejected
    draw is regenerated with the next seed, so nothing is left out."""
    if index not in _EXACT:
        case = exact_triangles.cases([EXACT_SPECS[index]])[0]
        assert exact_triangles.prove(case)
        assert np.array_equal(triangle_times(case, case.x), case.b)              # the restatement above is make()'s
        count = max(ALL_K if index < 2 else SOME_K)
        X = np.empty((case.n, count), np.int64)
        X[:, 0] = case.x
        for j in range(1, count):
            for attempt in range(50):
                x = np.random.default_rng([index, j, attempt]).integers(-900, 901, case.n)
                column = exact_triangles.Case(case.name, case.n, case.rp, case.ci, case.va, triangle_times(case, x), x,
                                              case.uplo, case.unit, case.widths)
                if exact_triangles.prove(column):
                    X[:, j] = x
                    break
            else:
                raise AssertionError(f"no provable column {j} for spec {index}")
        B = np.stack([triangle_times(case, X[:, j]) for j in range(count)], axis=1)
        assert (np.abs(B) < exact_triangles.LIMIT).all()
        _EXACT[index] = (case, B, X)
    return _EXACT[index]


def test_every_spec_has_its_columns():
    """nothing is left out: all six specs yield a proven case with all its proven columns (the columns are shared with
    the test below)"""
    for index in range(len(EXACT_SPECS)):
        case, B, X = exact_columns(index)
        count = max(ALL_K if index < 2 else SOME_K)
        assert B.shape == X.shape == (case.n, count)
        assert len({X[:, j].tobytes() for j in range(count)}) == count


@pytest.mark.parametrize("index", range(len(EXACT_SPECS)))
def test_exact_integer_systems_at_every_lane_count(gpu, monkeypatch, index):
    """sptrsv_multi_kernel<L, 4 | 8, WS, ordered> on levels wider than 256 rows, runs of narrow levels, 257 next to
    256, 30 levels in one launch, unit and power-of-two diagonals and both triangles: every column is the integer
    solution bit for bit, out of place and in place, and the launches are the single call's."""
    case, B_int, X_int = exact_columns(index)
    B_all, X_all = B_int.astype(np.float32), X_int.astype(np.float32)
    assert (B_all.astype(np.int64) == B_int).all() and (X_all.astype(np.int64) == X_int).all()
    dev = Device(gpu, case.n, case.rp, case.ci, case.va)
    kinds = set()
    try:
        for ordered, lanes in [(1, None)] + [(0, L) for L in LANES] + [(0, None)]:
            set_lanes(monkeypatch, lanes)
            cfg = gpu.SpTRSVConfig(uplo=case.uplo, diag=case.unit, ordered=ordered)
            ref, x_ref = dev.single(B_all[:, 0], cfg)
            assert ref.error_code == 0 and ref.num_levels == len(case.widths)
            assert lanes is None or ref.lanes_per_row == lanes
            np.testing.assert_array_equal(bits(x_ref), bits(X_all[:, 0]))
            for k in (ALL_K if index < 2 else SOME_K):
                for in_place in (False, True):
                    tag = (case.name, ordered, lanes, k, in_place)
                    res, X = dev.plain(B_all[:, :k], cfg, in_place=in_place)
                    same_shape(res, ref, tag)
                    np.testing.assert_array_equal(bits(X), bits(X_all[:, :k]), err_msg=str(tag))
            widths = np.array(case.widths)
            if (widths > NARROW).any():
                kinds.add("wide")
            if ref.launches < ref.num_levels:
                kinds.add("run")
    finally:
        set_lanes(monkeypatch, None)
        dev.close()
    want = {0: {"wide", "run"}, 1: {"wide", "run"}, 2: {"wide", "run"}, 3: {"wide", "run"}, 4: {"run"}, 5: {"wide"}}
    assert kinds == want[index]                      # both launch kinds were met (each alone in specs 4 and 5)


# ------------------------------------------------------------------------------------------ 2. inexact data
def _matrix(name, spd, nonsym):
    return {"poisson2d(64)": lambda: spd.poisson2d(64), "poisson3d(16)": lambda: spd.poisson3d(16),
            "random_spd(3000,15,3)": lambda: spd.random_spd(3000, 15, 3),
            "random_nonsym(3000,7,1)": lambda: nonsym.random_nonsym(3000, 7, 1)}[name]()


@pytest.mark.parametrize("name", ["poisson2d(64)", "poisson3d(16)", "random_spd(3000,15,3)",
                                  "random_nonsym(3000,7,1)"])
def test_columns_equal_the_single_call_bit_for_bit(gpu, spd, nonsym, monkeypatch, name):
    """Both triangles, both diagonal modes, every lane count and the ordered solve, k in {3, 8, 9, 32}: the columns
    of the largest batch are solved one by one once per configuration and shared by the smaller batches (their
    columns are its first ones)."""
    n, rp, ci, va = _matrix(name, spd, nonsym)
    dev = Device(gpu, n, rp, ci, va)
    B = np.random.default_rng(12).uniform(-1.0, 1.0, (n, K_MAX)).astype(np.float32)
    try:
        for uplo in (0, 1):
            for unit in (0, 1):
                for ordered, lanes in [(1, None)] + [(0, L) for L in LANES]:
                    set_lanes(monkeypatch, lanes)
                    cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit, ordered=ordered)
                    ref, X_ref = dev.singles(B, cfg)
                    assert ref.lanes_per_row == (1 if ordered else lanes)
                    if ordered:
                        with np.errstate(all="ignore"):
                            cpu = np.stack([gpu.sptrsv_cpu_csr(dev.A, B[:, j].copy(), cfg) for j in range(K_MAX)],
                                           axis=1)
                        assert_same_bits(X_ref, cpu, (name, uplo, unit, "cpu"))
                    for k in (3, 8, 9, 32):
                        tag = (name, uplo, unit, ordered, lanes, k)
                        res, X = dev.plain(B[:, :k], cfg)
                        same_shape(res, ref, tag)
                        assert_same_bits(X, X_ref[:, :k], tag)
    finally:
        set_lanes(monkeypatch, None)
        dev.close()


# ------------------------------------------------------------------------------------------ 3. layouts
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("k,ldb,ldx", [(5, 5, 5), (5, 8, 8), (5, 7, 6), (5, 8, 12), (9, 12, 16), (9, 11, 9), (4, 4, 8)])
def test_leading_dimensions_alignment_and_padding(gpu, spd, monkeypatch, k, ldb, ldx, offset):
    """16-byte accesses only where the view is aligned and the leading dimension a multiple of four, and only for whole
    groups of four columns below k; guarded scalar accesses everywhere else.  Device.multi asserts the poison in X's
    padding columns, around both arrays, and B itself; the arrays end at the last row's column k."""
    n, rp, ci, va = spd.random_spd(3000, 15, 3)
    dev = Device(gpu, n, rp, ci, va)
    B = np.random.default_rng(13).uniform(-1.0, 1.0, (n, k)).astype(np.float32)
    try:
        for uplo, lanes in ((0, 1), (1, 8), (0, 64)):
            set_lanes(monkeypatch, lanes)
            cfg = gpu.SpTRSVConfig(uplo=uplo)
            ref, X_ref = dev.singles(B, cfg)
            tag = (k, ldb, ldx, offset, uplo, lanes)
            res, X = dev.multi(B, cfg, ldb=ldb, ldx=ldx, offset=offset)
            same_shape(res, ref, tag)
            assert_same_bits(X, X_ref, tag)
            ld = max(ldb, ldx)
            res, X = dev.multi(B, cfg, ldb=ld, ldx=ld, offset=offset, in_place=True)     # in place with padding
            same_shape(res, ref, tag + ("in place",))
            assert_same_bits(X, X_ref, tag + ("in place",))
    finally:
        set_lanes(monkeypatch, None)
        dev.close()


# ------------------------------------------------------------------------------------------ 4. independence
def test_a_nan_column_and_a_zero_diagonal_stay_in_their_columns(gpu, spd, monkeypatch):
    n, rp, ci, va = spd.poisson2d(24)
    va = va.copy()
    r = np.repeat(np.arange(n), np.diff(rp))
    va[(ci == r) & (r == 300)] = 0.0
    dev = Device(gpu, n, rp, ci, va)
    k = 9
    B = np.random.default_rng(2).uniform(0.5, 1.0, (n, k)).astype(np.float32)
    B[:, 2] = np.nan
    B[:, 4] = 0.0                                                     # meets 0 / 0 at row 300, the others x / 0
    B[:300, 7] = 0.0
    try:
        for lanes in (1, 4, 64, None):
            for ordered in (0, 1):
                set_lanes(monkeypatch, lanes)
                cfg = gpu.SpTRSVConfig(uplo=0, ordered=ordered)
                ref, X_ref = dev.singles(B, cfg)
                res, X = dev.multi(B, cfg, ldx=k + 2)
                same_shape(res, ref, (lanes, ordered))
                assert_same_bits(X, X_ref, (lanes, ordered))
                assert np.isnan(X[:, 2]).all() and np.isnan(X[300, 4]) and not X[:300, 4].any()
                assert np.isinf(X[300, [0, 1, 3, 5, 6, 7, 8]]).all() and np.isfinite(X[:300, [0, 1, 3, 5, 6, 7, 8]]).all()
                if ordered:
                    with np.errstate(all="ignore"):
                        cpu = gpu.sptrsv_cpu_csr_multi(dev.A, B, cfg)
                    assert_same_bits(X, cpu, "cpu")
    finally:
        set_lanes(monkeypatch, None)
        dev.close()


def test_a_permutation_and_a_slice_of_the_columns_give_the_same_bits(gpu, nonsym, monkeypatch):
    n, rp, ci, va = nonsym.random_nonsym(3000, 7, 1)
    dev = Device(gpu, n, rp, ci, va)
    rng = np.random.default_rng(14)
    B = rng.uniform(-1.0, 1.0, (n, 16)).astype(np.float32)
    try:
        for uplo, lanes in ((0, 2), (1, 32), (1, None)):
            set_lanes(monkeypatch, lanes)
            cfg = gpu.SpTRSVConfig(uplo=uplo)
            _, X = dev.plain(B, cfg)
            perm = rng.permutation(16)
            _, Xp = dev.multi(B[:, perm], cfg, ldb=17, ldx=20)
            np.testing.assert_array_equal(bits(Xp), bits(X[:, perm]))
            _, Xs = dev.plain(B[:, 8:16], cfg)                        # the second window alone, as the first
            np.testing.assert_array_equal(bits(Xs), bits(X[:, 8:16]))
            _, X1 = dev.plain(B[:, 11:12], cfg)
            np.testing.assert_array_equal(bits(X1), bits(X[:, 11:12]))
    finally:
        set_lanes(monkeypatch, None)
        dev.close()


# ------------------------------------------------------------------------------------------ 5. reproducibility
def test_same_bits_across_runs_and_streams(gpu, spd, monkeypatch):
    import torch
    n, rp, ci, va = spd.random_spd(3000, 15, 3)
    dev = Device(gpu, n, rp, ci, va)
    k = 9
    B = np.random.default_rng(9).uniform(-1.0, 1.0, (n, k)).astype(np.float32)
    t_B = torch.from_numpy(B).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        for lanes in (None, 8, 64):
            set_lanes(monkeypatch, lanes)
            for uplo in (0, 1):
                cfg = gpu.SpTRSVConfig(uplo=uplo)
                assert gpu.sptrsv_analyze(dev.A, uplo).error_code == 0
                runs = [dev.plain(B, cfg)[1] for _ in range(3)]
                for other in runs[1:]:
                    np.testing.assert_array_equal(bits(other), bits(runs[0]))
                outs = [torch.full((n, k), float("nan"), device="cuda") for _ in streams]
                torch.cuda.synchronize()
                for st, out in zip(streams, outs):
                    assert gpu.sptrsv_csr_multi_async(dev.A, t_B.data_ptr(), out.data_ptr(), k, config=cfg,
                                                      stream=st.cuda_stream) == 0
                torch.cuda.synchronize()
                for out in outs:
                    np.testing.assert_array_equal(bits(out.cpu().numpy()), bits(runs[0]))
    finally:
        set_lanes(monkeypatch, None)
        dev.close()


def test_the_schedule_is_shared_with_the_single_call(gpu, spd):
    n, rp, ci, va = spd.random_spd(3000, 15, 3)
    dev = Device(gpu, n, rp, ci, va)
    B = np.random.default_rng(10).uniform(-1.0, 1.0, (n, 5)).astype(np.float32)
    lower, upper = gpu.SpTRSVConfig(uplo=0), gpu.SpTRSVConfig(uplo=1)
    try:
        first, _ = dev.plain(B, lower)                                 # the multi call analyses ...
        assert first.error_code == 0 and first.analysis_ms > 0
        single, _ = dev.single(B[:, 0], lower)                         # ... and the single call finds it
        assert single.analysis_ms == 0
        assert (single.num_levels, single.launches) == (first.num_levels, first.launches)
        assert dev.plain(B, lower)[0].analysis_ms == 0
        single, _ = dev.single(B[:, 0], upper)                         # the other way round, the other triangle
        assert single.error_code == 0 and single.analysis_ms > 0
        second, _ = dev.plain(B, upper)
        assert second.analysis_ms == 0 and (second.num_levels, second.launches) == (single.num_levels, single.launches)
        gpu.csr_invalidate_gpu_cache(dev.A)                            # dropped for both
        again, _ = dev.plain(B, lower)
        assert again.analysis_ms > 0 and dev.single(B[:, 0], lower)[0].analysis_ms == 0
        assert dev.single(B[:, 0], upper)[0].analysis_ms > 0 and dev.plain(B, upper)[0].analysis_ms == 0
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ 6. rejections
def test_rejections_leave_x_untouched(gpu, spd):
    E = gpu.SpMVError
    n, rp, ci, va = spd.poisson2d(24)
    r = np.repeat(np.arange(n), np.diff(rp))
    k = 5
    B = np.ones((n, k), np.float32)

    def rejected(dev, cfg, code, **layout):
        res, X = dev.multi(B, cfg, x_fill=-77.0, **layout)
        assert res.error_code == code, (res.error_code, code)
        assert (X == -77.0).all()

    keep = ~((ci == r) & (r == 100))                                  # row 100 loses its diagonal
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=n))]).astype(np.int32)
    dev = Device(gpu, n, rp2, ci[keep], va[keep])
    for uplo in (0, 1):
        for ordered in (0, 1):
            rejected(dev, gpu.SpTRSVConfig(uplo=uplo, diag=0, ordered=ordered), E.INVALID_ARGUMENT, ldx=7)
            res, X = dev.multi(B, gpu.SpTRSVConfig(uplo=uplo, diag=1, ordered=ordered), x_fill=-77.0)
            assert res.error_code == 0 and np.isfinite(X).all() and not (X == -77.0).any()      # UNIT needs none
    dev.close()
    bad = ci.copy()
    bad[50] = n + 5                                                   # a column outside [0, n)
    dev = Device(gpu, n, rp, bad, va)
    rejected(dev, gpu.SpTRSVConfig(), E.INVALID_FORMAT)
    dev.close()
    down = rp.copy()
    down[30] = down[29] - 1                                           # row_ptrs decrease
    dev = Device(gpu, n, down, ci, va)
    rejected(dev, gpu.SpTRSVConfig(uplo=1), E.INVALID_FORMAT, ldb=6)
    dev.close()
    # overlap on real device memory: partial, and in place with two leading dimensions
    dev = Device(gpu, n, rp, ci, va)
    ld = 8
    store = np.full(3 * n * ld, -77.0, np.float32)
    d = gpu.CudaBuffer(store.size)
    d.copyFromHost(store, store.size)
    base = d.get()
    for b_ptr, ldb, x_ptr, ldx in ((base, ld, base + 4 * 3, ld), (base + 4 * 3, ld, base, ld), (base, ld, base, ld - 1),
                                   (base, k, base, ld), (base, ld, base + 4 * ((n - 1) * ld + k - 1), ld)):
        res = gpu.sptrsv_csr_multi(dev.A, b_ptr, x_ptr, k, ldb, ldx)
        assert res.error_code == E.INVALID_ARGUMENT, (ldb, ldx)
        assert gpu.sptrsv_csr_multi_async(dev.A, b_ptr, x_ptr, k, ldb, ldx) == E.INVALID_ARGUMENT
        assert (d.copyToHost(store.size) == -77.0).all()
    assert gpu.sptrsv_csr_multi(dev.A, base, base + 4 * ((n - 1) * ld + k), k, ld, ld).error_code == 0   # they touch
    d.release()
    dev.close()


# ------------------------------------------------------------------------------------------ 7. C++ caller
def test_cpp_sptrsv_multi_smoke(gpu, tmp_path):
    """tests/cpp/sptrsv_multi_smoke.cpp through spmv/sptrsv.h, spmv/cg.h and CudaBuffer, compiled here with
    test_cpp_cg_multi_smoke's g++ line: both new device entry points and cg_solve_multi_ic."""
    exe = str(tmp_path / "sptrsv_multi_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "sptrsv_multi_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
