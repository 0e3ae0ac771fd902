"""The device-side level analysis (include/spmv/sptrsv.h sptrsv_analyze_device) on the GPU.  The
schedule is unique, so everything is held at zero tolerance: the device-built level pointers, order and statistics
against sptrsv_levels on the host arrays and against the host-built schedule of the same matrix, over structure
families that reach every launch kind and every switch between them; malformed input; determinism across builds and
streams; the shared cache; the solves and factorisations on a device-built schedule; the SPMV_DEBUG routing of the
implicit analyses; a C++ caller."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import sptrsv_analysis_cases as cases
from array_views import Views
from conftest import ROOT

pytestmark = pytest.mark.gpu

INFO_FIELDS = ("num_levels", "launches", "first_missing_diagonal", "first_unsorted_row", "one_sided_row",
               "built_on_device", "triangle_nnz")


@pytest.fixture(scope="module")
def spd():
    return importlib.import_module("gpu-spmv_amd.spd")


@pytest.fixture(scope="module")
def nonsym():
    return importlib.import_module("gpu-spmv_amd.nonsym")


@pytest.fixture(scope="module")
def families(spd, nonsym):
    """name -> (n, rp, ci, va), built once and never written"""
    built = cases.families(spd, nonsym)
    assert tuple(built) == cases.FAMILY_NAMES
    return built


def _upload(gpu, n, rp, ci, va):
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    return A


def _info(info):
    return {f: int(getattr(info, f)) for f in INFO_FIELDS}


def _device_schedule(gpu, A, uplo):
    res = gpu.sptrsv_analyze_device(A, uplo)
    assert res.error_code == 0 and res.analysis_ms > 0
    status, level_ptr, order, info = gpu.sptrsv_schedule_get(A, uplo)
    assert status == 0 and info.built_on_device == 1
    assert (res.num_levels, res.launches) == (info.num_levels, info.launches)
    return level_ptr, order, _info(info)


def _host_schedule(gpu, A, uplo):
    res = gpu.sptrsv_analyze(A, uplo)
    assert res.error_code == 0 and res.analysis_ms > 0
    status, level_ptr, order, info = gpu.sptrsv_schedule_get(A, uplo)
    assert status == 0 and info.built_on_device == 0
    return level_ptr, order, _info(info)


def _check_against_the_host(gpu, A, case, uplo, tag):
    """the device-built schedule of (A, uplo) against sptrsv_levels and against the host-built one; returns it"""
    n, rp, ci, _ = case
    gpu.csr_invalidate_gpu_cache(A)
    level_ptr, order, info = _device_schedule(gpu, A, uplo)
    status, want_ptr, want_order, want_levels, want_missing = gpu.sptrsv_levels(n, rp, ci, uplo)
    assert status == 0
    assert info["num_levels"] == want_levels and info["first_missing_diagonal"] == want_missing, (tag, info)
    np.testing.assert_array_equal(level_ptr, want_ptr, err_msg=str(tag))
    np.testing.assert_array_equal(order, want_order, err_msg=str(tag))
    assert info["launches"] == cases.launches(want_ptr), (tag, info)
    assert info["triangle_nnz"] == cases.triangle_nnz(n, rp, ci, uplo), (tag, info)
    assert info["first_unsorted_row"] == cases.first_unsorted_row(n, rp, ci), (tag, info)

    gpu.csr_invalidate_gpu_cache(A)
    assert gpu.sptrsv_schedule_get(A, uplo)[0] == gpu.SpMVError.INVALID_ARGUMENT
    host_ptr, host_order, host_info = _host_schedule(gpu, A, uplo)
    np.testing.assert_array_equal(level_ptr, host_ptr, err_msg=str(tag))
    np.testing.assert_array_equal(order, host_order, err_msg=str(tag))
    for f in INFO_FIELDS:
        if f not in ("built_on_device", "one_sided_row"):
            assert info[f] == host_info[f], (tag, f, info, host_info)
    assert (info["one_sided_row"] < 0) == (host_info["one_sided_row"] < 0), (tag, info, host_info)
    tested = uplo == 0 and info["first_missing_diagonal"] < 0 and info["first_unsorted_row"] < 0
    assert info["one_sided_row"] == (cases.one_sided_row(n, rp, ci) if tested else -1), (tag, info)
    gpu.csr_invalidate_gpu_cache(A)
    return level_ptr, order, info


# ---- the structure families --------------------------------------------------------------------------------------
@pytest.mark.parametrize("uplo", (0, 1))
@pytest.mark.parametrize("name", cases.FAMILY_NAMES)
def test_device_schedule_equals_the_host_schedule_int_for_int(gpu, families, name, uplo):
    case = families[name]
    A = _upload(gpu, *case)
    level_ptr, _, info = _check_against_the_host(gpu, A, case, uplo, (name, uplo))
    gpu.csr_destroy(A)
    widths = np.diff(level_ptr)
    n = case[0]
    if name.startswith("diagonal") or (name, uplo) == ("strictly lower(3000)", 1):
        assert widths.tolist() == [n]                            # one level, no dependents
    if name.startswith("chain"):
        assert widths.tolist() == [1] * n
    if name == "chain past the run limit":
        assert info["launches"] == 2
    if (name, uplo) in (("staircase", 0), ("staircase flipped", 1)):
        assert widths.tolist() == [255, 256, 257, 1, 600, 256]
    if name == "poisson2d(64)":
        assert widths.size == 127 and widths.max() == 64
    if name == "poisson3d(16)":
        assert widths.max() == 192
    if name == "poisson3d(32)":
        assert widths.max() > 2 * cases.NARROW
    if name == "arrow(5000)":
        assert widths.tolist() == ([1, n - 2, 1] if uplo == 0 else [n])
    if name == "messy(2000)":
        assert info["first_unsorted_row"] >= 0 and info["first_missing_diagonal"] >= 0
    if (name, uplo) in (("hub in a wide level", 0), ("hub in a wide level flipped", 1)):
        assert widths.tolist() == [300, n - 300]


LANES = (1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("lanes", LANES)
def test_every_lane_count_of_the_analysis_kernels(gpu, families, monkeypatch, lanes):
    """SPMV_DEBUG=analysis_lanes=N reaches every instantiation of the statistics, one-sided and peel kernels: narrow
    runs, wide levels, the switches between them, hubs in both launch kinds, unsorted rows and duplicates"""
    monkeypatch.setenv("SPMV_DEBUG", f"analysis_lanes={lanes}")
    for name in ("staircase", "staircase flipped", "poisson3d(16)", "messy(2000)", "arrow(5000)",
                 "hub in a wide level", "hub in a wide level flipped", "diagonal(257)", "n=2"):
        case = families[name]
        A = _upload(gpu, *case)
        for uplo in (0, 1):
            _check_against_the_host(gpu, A, case, uplo, (name, uplo, lanes))
        gpu.csr_destroy(A)


def test_views_at_odd_offsets_inside_larger_buffers(gpu, spd):
    case = spd.poisson3d(9)
    n, rp, ci, va = case
    for offsets in ((1, 2, 3), (3, 1, 0), (2, 3, 1)):
        with Views(gpu) as views:
            A, _ = views.csr(n, n, rp, ci, va, offsets)
            for uplo in (0, 1):
                _check_against_the_host(gpu, A, case, uplo, ("views", offsets, uplo))
            views.check_guards(("after the analyses", offsets))


def test_device_only_matrix_through_csr_wrap_device(gpu, nonsym):
    import torch
    case = nonsym.convdiff2d(40)
    n, rp, ci, va = case
    t_rp, t_ci, t_va = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, va))
    torch.cuda.synchronize()
    A = gpu.csr_wrap_device(n, n, int(ci.size), t_rp.data_ptr(), t_ci.data_ptr(), t_va.data_ptr())
    assert A is not None and not A.contents.owns_device_memory
    for uplo in (0, 1):
        _check_against_the_host(gpu, A, case, uplo, ("wrapped", uplo))
    gpu.csr_destroy(A)
    for t, a in ((t_rp, rp), (t_ci, ci)):
        np.testing.assert_array_equal(t.cpu().numpy(), a)                    # the structure is read, never written


# ---- malformed input ---------------------------------------------------------------------------------------------
def test_malformed_structures_are_rejected_and_nothing_is_cached(gpu, spd):
    E = gpu.SpMVError
    good = spd.poisson2d(20)
    n, rp, ci, va = good
    column_n, column_minus = ci.copy(), ci.copy()
    column_n[1234] = n
    column_minus[77] = -1
    down = rp.copy()
    down[30] = down[29] - 1
    past = rp.copy()
    past[n] = ci.size + 3                                          # row_ptrs[n] > nnz
    bad = {"a column equal to n": (rp, column_n), "a column of -1": (rp, column_minus),
           "a decreasing row pointer": (down, ci), "row_ptrs[n] > nnz": (past, ci)}
    G = _upload(gpu, *good)
    for what, (brp, bci) in bad.items():
        A = _upload(gpu, n, brp, bci, va)
        for uplo in (0, 1):
            res = gpu.sptrsv_analyze_device(A, uplo)
            assert res.error_code == E.INVALID_FORMAT and res.num_levels == 0, (what, uplo)
            assert gpu.sptrsv_schedule_get(A, uplo)[0] == E.INVALID_ARGUMENT, (what, uplo)
        gpu.csr_destroy(A)
        _check_against_the_host(gpu, G, good, 0, ("after", what))             # a valid matrix next is unaffected
    gpu.csr_destroy(G)


# ---- determinism -------------------------------------------------------------------------------------------------
def test_two_builds_and_a_build_on_a_second_stream_give_identical_arrays(gpu, families):
    import torch
    for name in ("poisson3d(32)", "messy(2000)", "staircase", "arrow(5000)"):
        A = _upload(gpu, *families[name])
        for uplo in (0, 1):
            first = _device_schedule(gpu, A, uplo)
            gpu.csr_invalidate_gpu_cache(A)
            again = _device_schedule(gpu, A, uplo)
            gpu.csr_invalidate_gpu_cache(A)
            stream = torch.cuda.Stream()
            try:
                gpu.set_stream(stream.cuda_stream)
                other = _device_schedule(gpu, A, uplo)
            finally:
                gpu.set_stream(None)
            gpu.csr_invalidate_gpu_cache(A)
            for got in (again, other):
                np.testing.assert_array_equal(got[0], first[0], err_msg=name)
                np.testing.assert_array_equal(got[1], first[1], err_msg=name)
                assert got[2] == first[2], name
        gpu.csr_destroy(A)


# ---- the cache ---------------------------------------------------------------------------------------------------
def test_one_cache_for_both_origins(gpu, spd):
    rng = np.random.default_rng(4)
    n, rp, ci, va = spd.poisson3d(12)
    A = _upload(gpu, n, rp, ci, va)
    k = 3
    d_b, d_x = gpu.CudaBuffer(n), gpu.CudaBuffer(n)
    d_B, d_X = gpu.CudaBuffer(n * k), gpu.CudaBuffer(n * k)
    d_b.copyFromHost(rng.uniform(-1, 1, n).astype(np.float32), n)
    d_B.copyFromHost(rng.uniform(-1, 1, n * k).astype(np.float32), n * k)
    for uplo in (0, 1):
        cfg = gpu.SpTRSVConfig(uplo=uplo)
        host = gpu.sptrsv_analyze(A, uplo)
        assert host.error_code == 0 and host.analysis_ms > 0
        assert gpu.sptrsv_analyze_device(A, uplo).analysis_ms == 0           # however built
        assert gpu.sptrsv_schedule_get(A, uplo, arrays=False)[3].built_on_device == 0
        gpu.csr_invalidate_gpu_cache(A)
        assert gpu.sptrsv_schedule_get(A, uplo)[0] == gpu.SpMVError.INVALID_ARGUMENT
        built = gpu.sptrsv_analyze_device(A, uplo)
        assert built.error_code == 0 and built.analysis_ms > 0
        assert (built.num_levels, built.launches) == (host.num_levels, host.launches)
        for res in (gpu.sptrsv_analyze(A, uplo), gpu.sptrsv_analyze_device(A, uplo),
                    gpu.sptrsv_csr(A, d_b, d_x, cfg), gpu.sptrsv_csr_multi(A, d_B, d_X, k, config=cfg)):
            assert res.error_code == 0 and res.analysis_ms == 0
            assert (res.num_levels, res.launches) == (host.num_levels, host.launches)
        assert gpu.sptrsv_schedule_get(A, uplo, arrays=False)[3].built_on_device == 1
        gpu.csr_invalidate_gpu_cache(A)                                      # drops the device-built one as well
        assert gpu.sptrsv_schedule_get(A, uplo)[0] == gpu.SpMVError.INVALID_ARGUMENT
    for buf in (d_b, d_x, d_B, d_X):
        buf.release()
    gpu.csr_destroy(A)


# ---- downstream: the consumers on a device-built schedule ------------------------------------------------------
def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_solves_and_factorisations_on_a_device_built_schedule_equal_the_cpu(gpu, spd, nonsym):
    rng = np.random.default_rng(8)
    for name, (n, rp, ci, va) in {"poisson2d(40)": spd.poisson2d(40), "convdiff3d(10)": nonsym.convdiff3d(10)}.items():
        A = _upload(gpu, n, rp, ci, va)
        b = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        d_b, d_x, d_f = gpu.CudaBuffer(n), gpu.CudaBuffer(n), gpu.CudaBuffer(ci.size)
        d_b.copyFromHost(b, n)
        for uplo in (0, 1):
            assert gpu.sptrsv_analyze_device(A, uplo).error_code == 0
            cfg = gpu.SpTRSVConfig(uplo=uplo, ordered=1)
            res = gpu.sptrsv_csr(A, d_b, d_x, cfg)
            assert res.error_code == 0 and res.analysis_ms == 0
            np.testing.assert_array_equal(_bits(d_x.copyToHost(n)), _bits(gpu.sptrsv_cpu_csr(A, b, cfg)), err_msg=name)
        assert gpu.sptrsv_schedule_get(A, 0, arrays=False)[3].built_on_device == 1
        res = gpu.ilu0_csr(A, d_f)
        assert res.error_code == 0 and res.analysis_ms == 0
        np.testing.assert_array_equal(_bits(d_f.copyToHost(ci.size)), _bits(gpu.ilu0_cpu_csr(A)[0]), err_msg=name)
        if name.startswith("poisson"):
            res = gpu.ic0_csr(A, d_f)
            assert res.error_code == 0 and res.analysis_ms == 0
            np.testing.assert_array_equal(_bits(d_f.copyToHost(ci.size)), _bits(gpu.ic0_cpu_csr(A)[0]), err_msg=name)
        for buf in (d_b, d_x, d_f):
            buf.release()
        gpu.csr_destroy(A)


def test_rejections_of_the_factorisations_on_a_device_built_schedule(gpu, spd, nonsym):
    E = gpu.SpMVError
    # a one-sided pattern: IC(0) rejects it before anything is written, ILU(0) takes it
    n, rp, ci, va = spd.poisson2d(20)
    r = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((r == 200) & (ci == 201))
    lop = cases.from_coo(n, r[keep], ci[keep])
    lop = (lop[0], lop[1], lop[2], va[keep])
    A = _upload(gpu, *lop)
    assert gpu.sptrsv_analyze_device(A, 0).error_code == 0
    info = gpu.sptrsv_schedule_get(A, 0, arrays=False)[3]
    assert info.built_on_device == 1 and info.one_sided_row == 201
    d_f = gpu.CudaBuffer(lop[2].size)
    d_f.copyFromHost(np.full(lop[2].size, -77.0, np.float32), lop[2].size)
    res = gpu.ic0_csr(A, d_f)
    assert res.error_code == E.INVALID_ARGUMENT and (d_f.copyToHost(lop[2].size) == -77.0).all()
    assert gpu.ilu0_csr(A, d_f).error_code == 0
    d_f.release()
    gpu.csr_destroy(A)
    # unsorted columns: ILU(0) rejects them
    case = cases.messy(nonsym, 400)
    A = _upload(gpu, *case)
    assert gpu.sptrsv_analyze_device(A, 0).error_code == 0
    assert gpu.sptrsv_schedule_get(A, 0, arrays=False)[3].first_unsorted_row >= 0
    d_f = gpu.CudaBuffer(case[2].size)
    d_f.copyFromHost(np.full(case[2].size, -77.0, np.float32), case[2].size)
    res = gpu.ilu0_csr(A, d_f)
    assert res.error_code == E.INVALID_ARGUMENT and (d_f.copyToHost(case[2].size) == -77.0).all()
    assert gpu.ic0_csr(A, d_f).error_code == E.INVALID_ARGUMENT
    d_f.release()
    gpu.csr_destroy(A)


# ---- implicit routing --------------------------------------------------------------------------------------------
def _preconditioned_runs(gpu, spd, nonsym):
    """[(what, built_on_device of both schedules, bits, iteration count)] of the four implicit analyses"""
    rng = np.random.default_rng(21)
    out = []
    for kind, (n, rp, ci, va) in (("ic", spd.poisson2d(24)), ("lu", nonsym.convdiff2d(24))):
        A = _upload(gpu, n, rp, ci, va)
        d_f, d_b, d_x = gpu.CudaBuffer(ci.size), gpu.CudaBuffer(n), gpu.CudaBuffer(n)
        res = (gpu.ic0_csr if kind == "ic" else gpu.ilu0_csr)(A, d_f)
        assert res.error_code == 0 and res.analysis_ms > 0
        origin = [gpu.sptrsv_schedule_get(A, 0, arrays=False)[3].built_on_device]
        out.append((kind + "0_csr", origin, _bits(d_f.copyToHost(ci.size)), res.num_levels))
        # the factor over A's structure arrays: a matrix of its own for the schedule cache (other values, same key)
        F = gpu.csr_wrap_device(n, n, int(ci.size), A.contents.d_row_ptrs, A.contents.d_col_indices, d_f.get())
        gpu.csr_invalidate_gpu_cache(A)                           # the solver's TriangularPair analyses both triangles
        d_b.copyFromHost(rng.uniform(-1.0, 1.0, n).astype(np.float32), n)
        d_x.copyFromHost(np.zeros(n, np.float32), n)
        if kind == "ic":
            res = gpu.cg_solve_ic(A, F, d_b, d_x, gpu.CGConfig(tolerance=1e-5, engine=0))
        else:
            res = gpu.bicgstab_solve_lu(A, F, d_b, d_x, gpu.BiCGStabConfig(tolerance=1e-5, engine=0))
        assert res.error_code == 0 and res.converged == 1
        origin = [gpu.sptrsv_schedule_get(F, u, arrays=False)[3].built_on_device for u in (0, 1)]
        out.append(("solve_" + kind, origin, _bits(d_x.copyToHost(n)), res.iterations))
        gpu.csr_destroy(F)
        for buf in (d_f, d_b, d_x):
            buf.release()
        gpu.csr_destroy(A)
    return out


def test_spmv_debug_routes_the_implicit_analyses_to_the_device(gpu, spd, nonsym, monkeypatch):
    monkeypatch.delenv("SPMV_DEBUG", raising=False)
    host = _preconditioned_runs(gpu, spd, nonsym)
    monkeypatch.setenv("SPMV_DEBUG", "sptrsv_analysis=device")
    device = _preconditioned_runs(gpu, spd, nonsym)
    monkeypatch.setenv("SPMV_DEBUG", "sptrsv_analysis=host")
    other = _preconditioned_runs(gpu, spd, nonsym)
    assert [w for w, _, _, _ in host] == ["ic0_csr", "solve_ic", "lu0_csr", "solve_lu"]
    for (what, h_origin, h_bits, h_count), (_, d_origin, d_bits, d_count), (_, o_origin, _, _) in zip(host, device, other):
        assert set(h_origin) == {0} and set(d_origin) == {1} and set(o_origin) == {0}, what
        np.testing.assert_array_equal(d_bits, h_bits, err_msg=what)
        assert d_count == h_count, what


# ---- C++ caller --------------------------------------------------------------------------------------------------
def test_cpp_sptrsv_analysis_smoke(gpu, tmp_path):
    """tests/cpp/sptrsv_analysis_smoke.cpp through spmv/sptrsv.h, spmv/ic0.h and CudaBuffer, compiled here with
    test_cpp_sptrsv_multi_smoke's g++ line."""
    exe = str(tmp_path / "sptrsv_analysis_smoke")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "sptrsv_analysis_smoke.cpp"),
                    "-L" + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-lspmv_amd", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + os.path.join(ROOT, "gpu-spmv_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib", "-w",
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr
