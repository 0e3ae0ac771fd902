"""sptrsv_csr (include/spmv/sptrsv.h) on the GPU: the ordered solve against sptrsv_cpu_csr bit for bit; every lane
count under the componentwise backward-error bound of substitution (no measured tolerance); integer systems proven
exact in any summation order (tests/exact_triangles.py) at zero tolerance; run-to-run and stream-to-stream bits; the
schedule cache; rejection before d_x is written; symmetric Gauss-Seidel composed from two solves; the C++ caller."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import exact_triangles
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LANES = (1, 2, 4, 8, 16, 32, 64)
NARROW = 256          # csrc/internal.h kSptrsvNarrowRows: the widest level a single workgroup takes inside a run


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


@pytest.fixture(scope="module")
def nonsym():
    return importlib.import_module("gpu-spmv_amd.nonsym")


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _assert_same_bits(got, want, tag=""):
    """bit for bit; where the CPU has a NaN (inf - inf once a UNIT solve overflows, or 0 / 0) the GPU must have one
    too, but a NaN's sign and payload are not compared: IEEE 754 leaves them open and x86 and gfx950 differ"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=tag)
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(_bits(got)[keep], _bits(want)[keep], err_msg=tag)


def _upload(gpu, n, rp, ci, va):
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    return A


def _solve(gpu, A, b, cfg, in_place=False, sentinel=None):
    n = A.contents.num_rows
    d_b = gpu.CudaBuffer(n)
    d_b.copyFromHost(b, n)
    d_x = d_b if in_place else gpu.CudaBuffer(n)
    if sentinel is not None and not in_place:
        d_x.copyFromHost(np.full(n, sentinel, np.float32), n)
    res = gpu.sptrsv_csr(A, d_b, d_x, cfg)
    x = d_x.copyToHost(n)
    d_b.release()
    if not in_place:
        d_x.release()
    return res, x


def _triangle(n, rp, ci, va, uplo, unit):
    """(rows, cols, vals) of T in fp64, the diagonal folded (NON_UNIT: fp32 storage-order sum) or set to 1 (UNIT),
    and the stored entries per row inside the triangle."""
    r = np.repeat(np.arange(n), np.diff(rp))
    off = (ci < r) if uplo == 0 else (ci > r)
    on = ci == r
    d = np.zeros(n, np.float32)
    for j in np.flatnonzero(on):
        d[r[j]] = np.float32(d[r[j]] + va[j])
    if unit:
        d[:] = 1.0
        length = np.bincount(r[off], minlength=n)
    else:
        length = np.bincount(r[off | on], minlength=n)
    rows = np.concatenate([r[off], np.arange(n)])
    cols = np.concatenate([ci[off], np.arange(n)])
    vals = np.concatenate([va[off].astype(np.float64), d.astype(np.float64)])
    return rows, cols, vals, length


def backward_error_ratio(n, rp, ci, va, b, x, uplo, unit):
    """max_i omega_i / gamma(len_i + 1), omega_i = |b - T x|_i / (|T||x| + |b|)_i in fp64"""
    rows, cols, vals, length = _triangle(n, rp, ci, va, uplo, unit)
    x64 = x.astype(np.float64)
    b64 = b.astype(np.float64)
    tx = np.bincount(rows, weights=vals * x64[cols], minlength=n)
    scale = np.bincount(rows, weights=np.abs(vals * x64[cols]), minlength=n) + np.abs(b64)
    omega = np.where(scale > 0, np.abs(b64 - tx) / np.where(scale > 0, scale, 1.0), 0.0)
    return float((omega / gamma(length + 1)).max())


def _matrices(spd, nonsym):
    return {"poisson2d(64)": spd.poisson2d(64), "poisson3d(16)": spd.poisson3d(16),
            "random_spd(20000,15,3)": spd.random_spd(20000, 15, 3), "random_nonsym": nonsym.random_nonsym(20000, 7, 1),
            "convdiff2d(48)": nonsym.convdiff2d(48), "convdiff3d(12)": nonsym.convdiff3d(12)}


# ---- bit-exact: ordered = 1 equals sptrsv_cpu_csr ------------------------------------------------------------
def test_ordered_solve_equals_the_cpu_bit_for_bit(gpu, spd, nonsym):
    rng = np.random.default_rng(3)
    saw_wide = saw_run = False
    for name, (n, rp, ci, va) in _matrices(spd, nonsym).items():
        A = _upload(gpu, n, rp, ci, va)
        b = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for uplo in (0, 1):
            _, level_ptr, _, levels, _ = gpu.sptrsv_levels(n, rp, ci, uplo)
            widths = np.diff(level_ptr)
            for unit in (0, 1):
                cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit, ordered=1)
                want = gpu.sptrsv_cpu_csr(A, b, cfg)
                for in_place in (False, True):
                    res, got = _solve(gpu, A, b, cfg, in_place=in_place)
                    tag = f"{name} uplo={uplo} unit={unit} in_place={in_place}"
                    assert res.error_code == 0 and res.lanes_per_row == 1 and res.num_levels == levels, tag
                    _assert_same_bits(got, want, tag)
                    assert 1 <= res.launches <= levels, tag
                    if ((widths[1:] <= NARROW) & (widths[:-1] <= NARROW)).any():     # two narrow levels in a row
                        assert res.launches < levels, tag
                        saw_run = True
                    if (widths > NARROW).any() and levels > 1:
                        assert res.launches > 1, tag
                        saw_wide = True
        gpu.csr_destroy(A)
    assert saw_wide and saw_run                  # both launch kinds ran


def test_ordered_solve_on_a_device_only_matrix(gpu, spd):
    import torch
    n, rp, ci, va = spd.random_spd(20000, 15, 3)
    host = gpu.csr_from_arrays(n, n, rp, ci, va)
    t_rp, t_ci, t_va = (torch.from_numpy(a).cuda() for a in (rp, ci, va))
    D = gpu.csr_wrap_device(n, n, int(ci.size), t_rp.data_ptr(), t_ci.data_ptr(), t_va.data_ptr())
    assert not D.contents.row_ptrs                                   # no host arrays at all
    b = np.random.default_rng(8).uniform(-1.0, 1.0, n).astype(np.float32)
    for uplo in (0, 1):
        cfg = gpu.SpTRSVConfig(uplo=uplo, ordered=1)
        res, got = _solve(gpu, D, b, cfg)
        assert res.error_code == 0 and res.analysis_ms > 0 and 1 < res.launches < res.num_levels
        np.testing.assert_array_equal(_bits(got), _bits(gpu.sptrsv_cpu_csr(host, b, cfg)))
    gpu.csr_destroy(D)
    gpu.csr_destroy(host)


# ---- backward error at every lane count ----------------------------------------------------------------------
def test_every_lane_count_meets_the_substitution_bound(gpu, spd, monkeypatch):
    """omega_i <= gamma(len_i + 1), u = 2^-24: the componentwise backward-error bound of substitution, which holds for
    any order of the row's sum; nothing here is measured and then allowed."""
    rng = np.random.default_rng(4)
    for name, (n, rp, ci, va) in (("poisson2d(64)", spd.poisson2d(64)), ("poisson3d(16)", spd.poisson3d(16)),
                                  ("random_spd(20000,15,3)", spd.random_spd(20000, 15, 3))):
        A = _upload(gpu, n, rp, ci, va)
        b = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        for uplo in (0, 1):
            for unit in (0, 1):
                cfg = gpu.SpTRSVConfig(uplo=uplo, diag=unit, ordered=0)
                for lanes in LANES + (None,):
                    if lanes is None:
                        monkeypatch.delenv("SPMV_DEBUG", raising=False)
                    else:
                        monkeypatch.setenv("SPMV_DEBUG", f"sptrsv_lanes={lanes}")
                    res, x = _solve(gpu, A, b, cfg)
                    tag = f"{name} uplo={uplo} unit={unit} lanes={lanes}"
                    assert res.error_code == 0, tag
                    assert res.lanes_per_row == (lanes if lanes is not None else res.lanes_per_row), tag
                    assert res.lanes_per_row in LANES, tag
                    assert np.isfinite(x).all(), tag
                    ratio = backward_error_ratio(n, rp, ci, va, b, x, uplo, unit)
                    print(f"{tag} lanes_used={res.lanes_per_row} omega/gamma={ratio:.3f}")
                    assert ratio <= 1.0, (tag, ratio)
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)


# ---- exact data, zero tolerance ------------------------------------------------------------------------------
EXACT_SPECS = [
    (1, 0, 0, [700, 40, 300, 5, 5, 5, 900, 257, 256, 10, 1, 1, 600]),      # wide levels and narrow runs, pow2 diagonal
    (2, 1, 0, [700, 40, 300, 5, 5, 5, 900, 257, 256, 10, 1, 1, 600]),
    (3, 0, 1, [300, 3, 3, 3, 1000, 17, 64, 65, 2]),                        # unit diagonal (stored 3 ignored)
    (4, 1, 1, [300, 3, 3, 3, 1000, 17, 64, 65, 2]),
    (5, 0, 0, [40] * 30),                                                  # one launch, 30 levels
    (6, 1, 0, [2000, 2000]),                                               # wide levels only
]


def test_exact_integer_systems_at_every_lane_count(gpu, monkeypatch):
    proven = exact_triangles.cases(EXACT_SPECS)
    assert len(proven) == len(EXACT_SPECS)                # nothing left out
    kinds = set()
    for case in proven:
        assert exact_triangles.prove(case)
        A = _upload(gpu, case.n, case.rp, case.ci, case.va)
        b = case.b.astype(np.float32)
        want = case.x.astype(np.float32)
        assert (b.astype(np.int64) == case.b).all() and (want.astype(np.int64) == case.x).all()
        for ordered, lanes in [(1, None)] + [(0, L) for L in LANES] + [(0, None)]:
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"sptrsv_lanes={lanes}")
            cfg = gpu.SpTRSVConfig(uplo=case.uplo, diag=case.unit, ordered=ordered)
            for in_place in (False, True):
                res, got = _solve(gpu, A, b, cfg, in_place=in_place)
                tag = f"{case.name} ordered={ordered} lanes={lanes} in_place={in_place}"
                assert res.error_code == 0 and res.num_levels == len(case.widths), tag
                if lanes is not None:
                    assert res.lanes_per_row == lanes, tag
                np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=tag)
                widths = np.array(case.widths[::-1] if case.uplo else case.widths)
                if (widths > NARROW).any():
                    kinds.add("wide")
                if res.launches < res.num_levels:
                    kinds.add("run")
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
    assert kinds == {"wide", "run"}


# ---- same bits -----------------------------------------------------------------------------------------------
def test_same_bits_across_runs_and_streams(gpu, spd, monkeypatch):
    import torch
    n, rp, ci, va = spd.random_spd(20000, 15, 3)
    A = _upload(gpu, n, rp, ci, va)
    b = np.random.default_rng(9).uniform(-1.0, 1.0, n).astype(np.float32)
    t_b = torch.from_numpy(b).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for lanes in (None, 8, 64):
        if lanes is None:
            monkeypatch.delenv("SPMV_DEBUG", raising=False)
        else:
            monkeypatch.setenv("SPMV_DEBUG", f"sptrsv_lanes={lanes}")
        for uplo in (0, 1):
            cfg = gpu.SpTRSVConfig(uplo=uplo)
            assert gpu.sptrsv_analyze(A, uplo).error_code == 0
            runs = [_solve(gpu, A, b, cfg)[1] for _ in range(3)]
            for other in runs[1:]:
                np.testing.assert_array_equal(_bits(other), _bits(runs[0]))
            outs = [torch.full((n,), float("nan"), device="cuda") for _ in streams]
            torch.cuda.synchronize()
            for st, out in zip(streams, outs):
                assert gpu.sptrsv_csr_async(A, t_b.data_ptr(), out.data_ptr(), cfg, st.cuda_stream) == 0
            torch.cuda.synchronize()
            for out in outs:
                np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(runs[0]))
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    gpu.csr_destroy(A)


# ---- cache ---------------------------------------------------------------------------------------------------
def test_schedule_cache(gpu, spd):
    n, rp, ci, va = spd.random_spd(20000, 15, 3)
    A = _upload(gpu, n, rp, ci, va)
    b = np.random.default_rng(10).uniform(-1.0, 1.0, n).astype(np.float32)
    lower, upper = gpu.SpTRSVConfig(uplo=0, ordered=1), gpu.SpTRSVConfig(uplo=1, ordered=1)
    first, x0 = _solve(gpu, A, b, lower)
    assert first.error_code == 0 and first.analysis_ms > 0
    second, x1 = _solve(gpu, A, b, lower)
    assert second.analysis_ms == 0 and (second.num_levels, second.launches) == (first.num_levels, first.launches)
    np.testing.assert_array_equal(_bits(x0), _bits(x1))
    # LOWER and UPPER schedules coexist
    up, xu = _solve(gpu, A, b, upper)
    assert up.error_code == 0 and up.analysis_ms > 0
    assert _solve(gpu, A, b, lower)[0].analysis_ms == 0 and _solve(gpu, A, b, upper)[0].analysis_ms == 0
    np.testing.assert_array_equal(_bits(xu), _bits(gpu.sptrsv_cpu_csr(A, b, upper)))
    assert gpu.sptrsv_analyze(A, 0).analysis_ms == 0 and gpu.sptrsv_analyze(A, 1).analysis_ms == 0
    # new values in place, same structure: the new matrix's solution, no invalidation, no analysis
    va2 = (va * np.float32(1.5) + np.where(va > 0, np.float32(0.25), np.float32(-0.125))).astype(np.float32)
    assert gpu.lib().spmv_c_memcpy_h2d(ctypes.c_void_p(A.contents.d_values), va2.ctypes.data_as(ctypes.c_void_p),
                                       va2.nbytes) == 0
    H = gpu.csr_from_arrays(n, n, rp, ci, va2)
    for cfg in (lower, upper):
        res, got = _solve(gpu, A, b, cfg)
        assert res.error_code == 0 and res.analysis_ms == 0
        np.testing.assert_array_equal(_bits(got), _bits(gpu.sptrsv_cpu_csr(H, b, cfg)))
    gpu.csr_destroy(H)
    # invalidation: the next call analyses again
    gpu.csr_invalidate_gpu_cache(A)
    again, _ = _solve(gpu, A, b, lower)
    assert again.analysis_ms > 0 and _solve(gpu, A, b, lower)[0].analysis_ms == 0
    ahead = gpu.sptrsv_analyze(A, 1)
    assert ahead.error_code == 0 and ahead.analysis_ms > 0 and ahead.num_levels == up.num_levels
    assert ahead.launches == up.launches and _solve(gpu, A, b, upper)[0].analysis_ms == 0
    gpu.csr_destroy(A)


# ---- rejection from the analysis -----------------------------------------------------------------------------
def test_rejections_from_the_analysis_leave_x_untouched(gpu, spd):
    E = gpu.SpMVError
    n, rp, ci, va = spd.poisson2d(24)
    r = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((ci == r) & (r == 100))                              # row 100 loses its diagonal
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r[keep], minlength=n))]).astype(np.int32)
    A = _upload(gpu, n, rp2, ci[keep], va[keep])
    b = np.ones(n, np.float32)
    for uplo in (0, 1):
        for ordered in (0, 1):
            res, x = _solve(gpu, A, b, gpu.SpTRSVConfig(uplo=uplo, diag=0, ordered=ordered), sentinel=-77.0)
            assert res.error_code == E.INVALID_ARGUMENT and (x == -77.0).all()
            res, x = _solve(gpu, A, b, gpu.SpTRSVConfig(uplo=uplo, diag=1, ordered=ordered), sentinel=-77.0)
            assert res.error_code == 0 and np.isfinite(x).all() and not (x == -77.0).any()      # UNIT needs none
    gpu.csr_destroy(A)
    bad = ci.copy()
    bad[50] = n + 5                                               # a column outside [0, n)
    A = _upload(gpu, n, rp, bad, va)
    res, x = _solve(gpu, A, b, gpu.SpTRSVConfig(), sentinel=-77.0)
    assert res.error_code == E.INVALID_FORMAT and (x == -77.0).all()
    gpu.csr_destroy(A)
    down = rp.copy()
    down[30] = down[29] - 1                                       # row_ptrs decrease
    A = _upload(gpu, n, down, ci, va)
    res, x = _solve(gpu, A, b, gpu.SpTRSVConfig(uplo=1), sentinel=-77.0)
    assert res.error_code == E.INVALID_FORMAT and (x == -77.0).all()
    gpu.csr_destroy(A)


def test_zero_diagonal_gives_the_ieee_quotient_like_the_cpu(gpu, spd):
    n, rp, ci, va = spd.poisson2d(24)
    va = va.copy()
    r = np.repeat(np.arange(n), np.diff(rp))
    va[(ci == r) & (r == 300)] = 0.0
    A = _upload(gpu, n, rp, ci, va)
    b = np.random.default_rng(2).uniform(0.5, 1.0, n).astype(np.float32)
    cfg = gpu.SpTRSVConfig(uplo=0, ordered=1)
    res, got = _solve(gpu, A, b, cfg)
    want = gpu.sptrsv_cpu_csr(A, b, cfg)
    assert res.error_code == 0 and not np.isfinite(want[300]) and np.isfinite(want[:300]).all()
    _assert_same_bits(got, want)
    gpu.csr_destroy(A)


# ---- composition: symmetric Gauss-Seidel ---------------------------------------------------------------------
def test_symmetric_gauss_seidel_from_two_solves(gpu, spd):
    """z = U^-1 (D o (L^-1 r)) on the full poisson2d(32) matrix: each solve under the substitution bound against its
    own right-hand side, and z against the fp64 dense computation within what the two bounds allow."""
    n, rp, ci, va = spd.poisson2d(32)
    A = _upload(gpu, n, rp, ci, va)
    dense = np.zeros((n, n), np.float64)
    dense[np.repeat(np.arange(n), np.diff(rp)), ci] = va
    L, Up, D = np.tril(dense), np.triu(dense), np.diag(dense).copy()
    r = np.random.default_rng(6).uniform(-1.0, 1.0, n).astype(np.float32)
    d_r, d_y, d_z = gpu.CudaBuffer(n), gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_r.copyFromHost(r, n)
    res = gpu.sptrsv_csr(A, d_r, d_y, gpu.SpTRSVConfig(uplo=0))
    assert res.error_code == 0
    y = d_y.copyToHost(n)
    w = (y * D.astype(np.float32)).astype(np.float32)                 # the element-wise scale, one rounding
    d_y.copyFromHost(w, n)
    res = gpu.sptrsv_csr(A, d_y, d_z, gpu.SpTRSVConfig(uplo=1))
    assert res.error_code == 0
    z = d_z.copyToHost(n)
    assert backward_error_ratio(n, rp, ci, va, r, y, 0, 0) <= 1.0
    assert backward_error_ratio(n, rp, ci, va, w, z, 1, 0) <= 1.0
    # forward error from the backward errors: |x^ - x| <= |T^-1| (gamma |T||x^| + gamma |b|) per solve, in fp64
    g = gamma(np.diff(rp).max() + 1)
    y64 = np.linalg.solve(L, r.astype(np.float64))
    z64 = np.linalg.solve(Up, D * y64)
    Li, Ui = np.abs(np.linalg.inv(L)), np.abs(np.linalg.inv(Up))
    dy = Li @ (g * (np.abs(L) @ np.abs(y) + np.abs(r)))
    dw = np.abs(D) * dy + U * np.abs(D * y)
    dz = Ui @ (g * (np.abs(Up) @ np.abs(z) + np.abs(w)) + dw)
    assert (np.abs(y - y64) <= dy).all()
    assert (np.abs(z - z64) <= dz).all()
    for buf in (d_r, d_y, d_z):
        buf.release()
    gpu.csr_destroy(A)


def test_cpp_sptrsv_caller(gpu):
    exe = os.path.join(ROOT, "tests", "cpp", "bin", "sptrsv_smoke")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
