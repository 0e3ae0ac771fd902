"""Reverse Cuthill-McKee (include/spmv/reorder.h) on the host side (no GPU): the exported names and struct layouts;
csr_rcm_cpu against both restatements of the header in tests/rcm_cases.py at zero tolerance, for every graph as
generated and shuffled, with and without the pseudo-peripheral search and the symmetry promise; csr_band_cpu against
numpy; the figures recorded in tests/golden/rcm_restate.json against a fresh run; every rejection in the stated order
with the outputs untouched; and csrc/rcm_host.cpp under AddressSanitizer + UBSan through a stand-alone caller."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import rcm_cases as cases
import reorder_cases as rc
from conftest import ROOT

PERM, INV = 0x900000, 0xA00000                          # fake, never-dereferenced device addresses
FAKE_RP, FAKE_CI, FAKE_VA = 0x500000, 0x600000, 0x700000
NAMES = ("csr_rcm", "csr_rcm_cpu", "rcm_reorder", "csr_band_gpu", "csr_band_cpu")


def test_names_exist_in_the_header_the_c_abi_the_library_and_python(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    public = open(os.path.join(ROOT, "include", "spmv", "reorder.h")).read()
    for name in NAMES:
        assert "spmv_c_" + name in spmv.EXPORTED_SYMBOLS and hasattr(spmv.lib(), "spmv_c_" + name)
        assert "spmv_c_" + name + "(" in header and callable(getattr(spmv, name))
        assert " " + name + "(" in public
    assert "bandwidth(" not in public                     # that word is bandwidth.h's


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R, B = spmv.RcmConfig, spmv.RcmResult, spmv.CsrBand
    assert (ctypes.sizeof(C), ctypes.sizeof(R), ctypes.sizeof(B)) == (16, 24, 16)
    assert [f for f, _ in C._fields_] == ["symmetric_pattern", "peripheral", "lanes_per_row", "reserved"]
    assert [f for f, _ in R._fields_] == ["error_code", "components", "levels", "sweeps", "launches", "elapsed_ms"]
    assert [f for f, _ in B._fields_] == ["lower", "upper", "profile"]
    assert [getattr(C, f).offset for f, _ in C._fields_] == [0, 4, 8, 12]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 20]
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8]
    c = C()
    assert (c.symmetric_pattern, c.peripheral, c.lanes_per_row, c.reserved) == (0, 1, 0, 0)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_csr_rcm_cpu_is_both_restatements(spmv, name):
    n, rp, ci, va = cases.CASES[name]()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    for peripheral in (0, 1):
        for promised in (0, 1):
            want = cases.rcm_queue(n, rp, ci, peripheral, promised)
            by_level = cases.rcm_levels(n, rp, ci, peripheral, promised)
            assert np.array_equal(want[0], by_level[0]) and want[2:] == by_level[2:], (name, peripheral, promised)
            status, perm, inverse, components, levels = spmv.csr_rcm_cpu(
                A, spmv.RcmConfig(symmetric_pattern=promised, peripheral=peripheral))
            assert status == 0
            assert np.array_equal(perm, want[0]), (name, peripheral, promised)
            assert np.array_equal(inverse, want[1]), (name, peripheral, promised)
            assert (components, levels) == want[2:], (name, peripheral, promised)
            assert np.array_equal(np.sort(perm), np.arange(n)) and np.array_equal(inverse[perm], np.arange(n))
    # a null config is (0, 1, 0, 0)
    assert np.array_equal(spmv.csr_rcm_cpu(A)[1], cases.rcm_queue(n, rp, ci)[0])
    spmv.csr_destroy(A)


def test_isolated_vertices_come_first_in_index_order_before_the_reversal(spmv):
    n, rp, ci, va = cases.block_mix()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, perm, inverse, components, levels = spmv.csr_rcm_cpu(A)
    assert status == 0 and components == 8
    assert perm[::-1][:4].tolist() == [0, 4, 9, 14]
    # then the components by their vertex of smallest (degree, index): the path (5), the star (16), the triangle, K4
    sequence = perm[::-1].tolist()
    assert [sorted(sequence[a:b]) for a, b in ((4, 8), (8, 12), (12, 15), (15, 19))] == [
        [5, 6, 7, 8], [15, 16, 17, 18], [1, 2, 3], [10, 11, 12, 13]]
    assert levels == 4 + 4 + 3 + 2 + 2
    spmv.csr_destroy(A)


def test_a_broken_symmetry_promise_gives_a_defined_permutation(spmv):
    n, rp, ci, va = rc.upper_bidiagonal(40)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, honest, inverse, components, levels = spmv.csr_rcm_cpu(A)
    assert status == 0 and (components, levels) == (1, 40) and max(cases.band(n, rp, ci, inverse)[:2]) == 1
    status, promised, _, components, _ = spmv.csr_rcm_cpu(A, spmv.RcmConfig(symmetric_pattern=1))
    assert status == 0 and np.array_equal(promised, cases.rcm_queue(n, rp, ci, 1, 1)[0])
    assert np.array_equal(np.sort(promised), np.arange(n)) and components > 1
    spmv.csr_destroy(A)


BAND_CASES = {
    "rectangular": lambda: rc.with_row_lengths([3, 0, 17, 1, 64, 5, 65, 9, 0, 33] * 3 + [7] * 7, 91, seed=1),
    "wide": lambda: rc.with_row_lengths([5, 0, 0, 2], 600, seed=3),
    "tall": lambda: rc.with_row_lengths([2] * 300, 7, seed=4),
    "no entries": lambda: rc.with_row_lengths([0] * 9, 9, seed=5),
}


@pytest.mark.parametrize("name", list(BAND_CASES) + list(cases.LIBRARY))
def test_csr_band_cpu_is_numpy(spmv, name):
    if name in BAND_CASES:
        rows, cols, rp, ci, va = BAND_CASES[name]()
    else:
        rows, rp, ci, va = cases.shuffle(cases.LIBRARY[name](), 2)
        cols = rows
    A = spmv.csr_from_arrays(rows, cols, rp, ci, va)
    assert spmv.csr_band_cpu(A) == (0,) + cases.band(rows, rp, ci)
    spmv.csr_destroy(A)


def test_recorded_figures_against_a_fresh_run(spmv):
    with open(os.path.join(ROOT, "tests", "golden", cases.GOLDEN)) as f:
        recorded = json.load(f)
    assert set(recorded) == set(cases.RECORDED)
    for name, make in cases.RECORDED.items():
        n, rp, ci, va = make()
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        status, perm, inverse, components, levels = spmv.csr_rcm_cpu(A)
        assert status == 0
        B = spmv.csr_create(0, 0, 0)
        assert spmv.csr_permute_cpu(B, A, perm, inverse) == 0
        fresh = {"before": list(spmv.csr_band_cpu(A)[1:]), "after": list(spmv.csr_band_cpu(B)[1:]),
                 "components": components, "levels": levels}
        print(name, fresh)
        assert recorded[name] == fresh
        if n <= 1100:                                    # the restatement itself, where it is quick
            assert cases.record(name) == fresh
        spmv.csr_destroy(A)
        spmv.csr_destroy(B)
    for name, (before, after) in cases.QUOTED.items():
        assert max(recorded[name]["before"][:2]) == before and max(recorded[name]["after"][:2]) == after
    for name, (before, after) in cases.QUOTED_PROFILE.items():
        assert recorded[name]["before"][2] == before and recorded[name]["after"][2] == after


def test_host_rejections_in_order_with_the_outputs_untouched(spmv):
    E = spmv.SpMVError
    Cfg = spmv.RcmConfig
    n, rp, ci, va = rc.path(6)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    R = spmv.csr_create(3, 4, 0)
    Z = spmv.csr_create(0, 0, 0)
    perm, inverse = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    bad = Cfg(lanes_per_row=3, peripheral=7, reserved=9)

    def call(M, cfg=None):
        return spmv.csr_rcm_cpu(M, cfg, perm, inverse)[0]

    assert call(None, bad) == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_rcm_cpu(A, None, inverse.ctypes.data, None, None, None) == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_rcm_cpu(A, perm.ctypes.data, None, None, None, None) == E.INVALID_ARGUMENT
    assert call(R, bad) == E.INVALID_DIMENSION
    assert spmv.csr_rcm_cpu(Z, bad)[3:] == (0, 0)        # no rows: SUCCESS before the config is looked at
    for cfg in (Cfg(lanes_per_row=3), Cfg(lanes_per_row=128), Cfg(lanes_per_row=-2), Cfg(peripheral=2),
                Cfg(peripheral=-1), Cfg(reserved=1)):
        assert call(A, cfg) == E.INVALID_ARGUMENT
    bad_ci = ci.copy()
    bad_ci[4] = n
    M = spmv.csr_from_arrays(n, n, rp, bad_ci, va)
    assert call(M) == E.INVALID_FORMAT and call(M, bad) == E.INVALID_ARGUMENT      # the config comes first
    mn, mrp, mci, mva = rc.messy()
    X = spmv.csr_from_arrays(mn, mn, mrp, mci, mva)
    assert spmv.csr_rcm_cpu(X)[0] == E.INVALID_FORMAT                               # unsorted, repeated
    for make in cases.RAW.values():                                                 # as the generators leave them
        rn, rrp, rci, rva = make()
        W = spmv.csr_from_arrays(rn, rn, rrp, rci, rva)
        assert spmv.csr_rcm_cpu(W)[0] == E.INVALID_FORMAT
        spmv.csr_destroy(W)
    assert np.all(perm == -7) and np.all(inverse == -7)
    assert spmv.csr_band_cpu(None)[0] == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_band_cpu(A, None) == E.INVALID_ARGUMENT
    assert spmv.csr_band_cpu(M)[0] == E.INVALID_FORMAT
    assert spmv.csr_band_cpu(X)[0] == 0                                             # unsorted rows are fine there
    for Y in (A, R, Z, M, X):
        spmv.csr_destroy(Y)


def test_device_entry_points_check_before_any_device_work(spmv):
    """every call below must return before it touches a (fake) device address"""
    E = spmv.SpMVError
    Cfg = spmv.RcmConfig
    bad = Cfg(lanes_per_row=3, peripheral=7, reserved=9)
    D = spmv.csr_wrap_device(100, 100, 300, FAKE_RP, FAKE_CI, FAKE_VA)
    n, rp, ci, va = rc.path(6)
    H = spmv.csr_from_arrays(n, n, rp, ci, va)                                          # host only
    R = spmv.csr_wrap_device(5, 4, 0, FAKE_RP, FAKE_CI, FAKE_VA)
    Z = spmv.csr_create(0, 0, 0)
    B = spmv.csr_create(0, 0, 0)
    assert spmv.csr_rcm(None, PERM, INV, bad).error_code == E.INVALID_ARGUMENT
    assert spmv.csr_rcm(D, None, INV, bad).error_code == E.INVALID_ARGUMENT
    assert spmv.csr_rcm(D, PERM, None, bad).error_code == E.INVALID_ARGUMENT
    assert spmv.csr_rcm(R, PERM, INV, bad).error_code == E.INVALID_DIMENSION
    res = spmv.csr_rcm(Z, PERM, INV, bad)
    assert (res.error_code, res.components, res.levels, res.sweeps, res.launches) == (0, 0, 0, 0, 0)
    assert spmv.csr_rcm(H, PERM, INV, bad).error_code == E.INVALID_FORMAT
    for rp_, ci_, va_ in ((FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
        M = spmv.csr_wrap_device(8, 8, 16, rp_, ci_, va_)
        assert spmv.csr_rcm(M, PERM, INV, bad).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(M)
    for cfg in (Cfg(lanes_per_row=3), Cfg(lanes_per_row=-1), Cfg(lanes_per_row=128), Cfg(peripheral=2),
                Cfg(peripheral=-1), Cfg(reserved=1), bad):
        assert spmv.csr_rcm(D, PERM, INV, cfg).error_code == E.INVALID_ARGUMENT
    # rcm_reorder: its own nulls and B == A, then csr_rcm's
    assert spmv.rcm_reorder(None, D, PERM, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.rcm_reorder(B, None, PERM, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.rcm_reorder(B, D, None, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.rcm_reorder(B, D, PERM, None).error_code == E.INVALID_ARGUMENT
    assert spmv.rcm_reorder(D, D, PERM, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.rcm_reorder(B, R, PERM, INV).error_code == E.INVALID_DIMENSION
    assert spmv.rcm_reorder(B, D, PERM, INV, Cfg(reserved=1)).error_code == E.INVALID_ARGUMENT
    assert (B.contents.num_rows, B.contents.nnz) == (0, 0)
    # csr_band_gpu
    assert spmv.csr_band_gpu(None)[0] == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_band_gpu(D, None) == E.INVALID_ARGUMENT
    assert spmv.csr_band_gpu(H)[0] == E.INVALID_FORMAT
    for X in (D, H, R, Z, B):
        spmv.csr_destroy(X)


def test_rcm_host_under_sanitizers():
    """make -C gpu-spmv_amd sanitize-rcm builds tests/cpp/bin/rcm_host_sanitized (csrc/rcm_host.cpp and
    tests/cpp/rcm_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-rcm"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "rcm_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
