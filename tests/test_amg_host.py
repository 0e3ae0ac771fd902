"""The aggregation AMG (include/spmv/amg.h) on the host side (no GPU): the exported names and the struct layouts;
amg_aggregate_cpu_csr against the numpy restatement of its three passes, entry for entry; the partition properties;
the level sizes of the restated hierarchy; every check that needs no device, with fake device addresses that must
never be dereferenced; the exact prover's verdicts; and the sanitized caller."""
import ctypes
import importlib
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import amg_cases as ac
from conftest import ROOT

spd = importlib.import_module("gpu-spmv_amd.spd")

NAMES = ("amg_setup", "amg_update", "amg_destroy", "amg_num_levels", "amg_level", "amg_apply",
         "amg_aggregate_cpu_csr", "cg_solve_amg")
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def diagonal_matrix(n):
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(1, 2, n).astype(np.float32)


CASES = {
    "poisson2d(5)": (lambda: spd.poisson2d(5), 0.08),
    "poisson2d(16)": (lambda: spd.poisson2d(16), 0.08),
    "poisson3d(5)": (lambda: spd.poisson3d(5), 0.08),
    "random_spd(300, 7)": (lambda: spd.random_spd(300, 7), 0.08),
    "diagonal": (lambda: diagonal_matrix(37), 0.08),
    "theta = 0": (lambda: spd.random_spd(300, 7), 0.0),
    "poisson theta = 0": (lambda: spd.poisson2d(16), 0.0),
    "nothing strong": (lambda: spd.poisson2d(16), 0.5),
    "nothing strong, random": (lambda: spd.random_spd(300, 7), 10.0),
}


# ---- names and layouts ---------------------------------------------------------------------------------------
def test_names_in_the_headers_the_library_and_the_python_mirror(spmv):
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    declared = set(re.findall(r"\b(spmv_c_[a-z0-9_]+)\s*\(", header))
    assert declared == set(spmv.EXPORTED_SYMBOLS)
    cxx = open(os.path.join(ROOT, "include", "spmv", "amg.h")).read() + \
        open(os.path.join(ROOT, "include", "spmv", "cg.h")).read()
    for name in NAMES:
        c_name = "spmv_c_" + name
        assert c_name in declared and c_name in spmv.EXPORTED_SYMBOLS, name
        assert hasattr(spmv.lib(), c_name) and callable(getattr(spmv, name)), name
        assert re.search(r"\b%s\s*\(" % name, cxx), name


def test_struct_layouts_and_defaults(spmv):
    C, R = spmv.AMGConfig, spmv.AMGResult
    assert ctypes.sizeof(C) == 28 and ctypes.sizeof(R) == 48
    assert [getattr(C, f).offset for f, _ in C._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    c = C()
    assert (c.max_levels, c.coarse_rows, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps) == (10, 64, 1, 1, 4)
    assert c.strength == np.float32(0.08) and c.jacobi_weight == np.float32(2.0) / np.float32(3.0)


# ---- the aggregation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_aggregation_equals_the_restatement_entry_for_entry(spmv, name):
    make, theta = CASES[name]
    n, rp, ci, va = make()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    try:
        status, agg, count = spmv.amg_aggregate_cpu_csr(A, theta)
        want, want_count = ac.aggregate(n, rp, ci, va, theta)
        assert status == 0 and count == want_count, (name, count, want_count)
        np.testing.assert_array_equal(agg, want)
        # a partition with dense numbers, and the same arrays from a second call
        assert agg.min() == 0 and np.array_equal(np.unique(agg), np.arange(count))
        status2, agg2, count2 = spmv.amg_aggregate_cpu_csr(A, theta)
        assert (status2, count2) == (0, count) and np.array_equal(agg, agg2)
        if name in ("diagonal", "nothing strong", "nothing strong, random"):
            assert count == n and np.array_equal(agg, np.arange(n))           # all singletons, in row order
        else:
            assert count < n
    finally:
        spmv.csr_destroy(A)


def test_random_spd_has_unsorted_rows_and_repeated_columns():
    n, rp, ci, va = spd.random_spd(300, 7)
    unsorted = repeated = False
    for i in range(n):
        row = ci[rp[i]:rp[i + 1]]
        unsorted |= bool((np.diff(row) < 0).any())
        repeated |= np.unique(row).size < row.size
    assert unsorted and repeated


def test_second_pass_takes_the_largest_entry_and_the_first_on_a_tie(spmv):
    # rows 0 and 3 open the aggregates {0, 1} and {3, 4}; row 2 is left over with the strong neighbours 1 and 4
    def matrix(left, right):
        dense = np.diag(np.full(5, 4.0, np.float32))
        for i, j, v in ((0, 1, -2.0), (1, 2, left), (2, 4, right), (3, 4, -2.0)):
            dense[i, j] = dense[j, i] = v
        rows, cols = np.nonzero(dense)
        rp = np.zeros(6, np.int32)
        np.cumsum(np.bincount(rows, minlength=5), out=rp[1:])
        return 5, rp, cols.astype(np.int32), dense[rows, cols]

    for left, right, want in ((-1.0, -1.5, 1), (-1.5, -1.0, 0), (-1.0, -1.0, 0), (1.0, -1.0, 0)):
        n, rp, ci, va = matrix(left, right)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        status, agg, count = spmv.amg_aggregate_cpu_csr(A, 0.08)
        spmv.csr_destroy(A)
        assert status == 0 and count == 2 and agg.tolist() == [0, 0, want, 1, 1], (left, right, agg)
        np.testing.assert_array_equal(agg, ac.aggregate(n, rp, ci, va, 0.08)[0])


def test_level_sizes_of_the_restated_hierarchy(spmv):
    """theta = 0.08, coarse_rows = 64: the sizes come out of the restatement, and they are the ones the design
    prototype gave (a cross-check of the restatement, not constants the library is held to)."""
    sizes = {}
    for name, make in (("poisson2d(16)", lambda: spd.poisson2d(16)), ("poisson2d(32)", lambda: spd.poisson2d(32)),
                       ("poisson3d(8)", lambda: spd.poisson3d(8))):
        levels = ac.hierarchy(spmv, *make())
        sizes[name] = [level["n"] for level in levels]
        for level in levels[:-1]:
            assert level["count"] == levels[levels.index(level) + 1]["n"]
        assert sizes[name][-1] <= 64 and all(s > 64 for s in sizes[name][:-1])
    assert sizes == {"poisson2d(16)": [256, 48], "poisson2d(32)": [1024, 176, 24], "poisson3d(8)": [512, 72, 14]}


def test_pair_aggregates_halve_the_tridiagonal_matrix(spmv):
    n, rp, ci, va = ac.tridiagonal(56)
    levels = ac.hierarchy(spmv, n, rp, ci, va, maps=ac.pair_maps(56, 7))
    assert [level["n"] for level in levels] == [56, 28, 14, 7]
    for level in levels:
        want = ac.tridiagonal(level["n"])
        for got, expected in zip((level["rp"], level["ci"], level["va"]), want[1:]):
            np.testing.assert_array_equal(got, expected)


# ---- the prover ------------------------------------------------------------------------------------------------
def test_the_prover_admits_the_three_cases_and_rejects_large_inputs():
    for n, coarsest in ((24, 3), (28, 7), (56, 7)):
        r = ac.exact_rhs(n)
        z, width = ac.prove_vcycle(n, coarsest, r, 0.5, 1)
        assert z is not None and width <= 24, (n, width)
        # the cycle is close to the solve: the fp64 restatement agrees with the exact answer
        sizes = [n]
        while sizes[-1] > coarsest:
            sizes.append(sizes[-1] // 2)
        levels = [dict(zip(("n", "rp", "ci", "va"), ac.tridiagonal(m)), agg=None, count=0) for m in sizes]
        for level in levels[:-1]:
            level["agg"], level["count"] = (np.arange(level["n"]) // 2).astype(np.int32), level["n"] // 2
        z64 = ac.vcycle(levels, r, omega=0.5, pre=1, post=1, dtype=np.float64)
        assert np.max(np.abs(z64 - z.astype(np.float64))) <= 1e-12 * max(1.0, float(np.abs(z).max()))
    z, why = ac.prove_vcycle(28, 7, ac.exact_rhs(28) * np.float32(1 << 22), 0.5, 1)
    assert z is None and "bits" in why
    z, why = ac.prove_vcycle(28, 7, ac.exact_rhs(28), Fraction(1, 3), 1)
    assert z is None and why == "not dyadic"


# ---- rejections without a device -------------------------------------------------------------------------------
def test_aggregate_checks_in_the_stated_order_with_nothing_written(spmv):
    E = spmv.SpMVError
    lib = spmv.lib()
    f32 = lambda v: np.asarray(v, np.float32)
    A = spmv.csr_from_arrays(3, 3, [0, 2, 3, 5], [0, 1, 1, 1, 2], f32([2, -1, 2, -1, 2]))
    R = spmv.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], f32([1, 1]))
    agg = np.full(3, -7, np.int32)
    count = ctypes.c_int32(-7)
    ptr = agg.ctypes.data_as(ctypes.c_void_p)
    assert lib.spmv_c_amg_aggregate_cpu_csr(None, 0.08, ptr, ctypes.byref(count)) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_aggregate_cpu_csr(A, 0.08, None, ctypes.byref(count)) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_aggregate_cpu_csr(A, 0.08, ptr, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_aggregate_cpu_csr(R, -1.0, ptr, ctypes.byref(count)) == E.INVALID_DIMENSION
    for rp, ci in (([0, 2, 3, 4], [0, 1, 1, 1, 2]), ([1, 2, 3, 5], [0, 1, 1, 1, 2]), ([0, 3, 2, 5], [0, 1, 1, 1, 2]),
                   ([0, 2, 3, 5], [0, 1, 1, 3, 2]), ([0, 2, 3, 5], [0, -1, 1, 1, 2])):
        X = spmv.csr_from_arrays(3, 3, rp, ci, f32([2, -1, 2, -1, 2]))
        assert lib.spmv_c_amg_aggregate_cpu_csr(X, -1.0, ptr, ctypes.byref(count)) == E.INVALID_FORMAT, (rp, ci)
        spmv.csr_destroy(X)
    D = spmv.csr_wrap_device(3, 3, 5, FAKE_RP, FAKE_CI, FAKE_VA)                 # no host arrays
    assert lib.spmv_c_amg_aggregate_cpu_csr(D, 0.08, ptr, ctypes.byref(count)) == E.INVALID_FORMAT
    for theta in (-0.5, float("nan")):
        assert lib.spmv_c_amg_aggregate_cpu_csr(A, theta, ptr, ctypes.byref(count)) == E.INVALID_ARGUMENT
    assert count.value == -7 and (agg == -7).all()
    assert lib.spmv_c_amg_aggregate_cpu_csr(A, 0.08, ptr, ctypes.byref(count)) == 0 and count.value >= 1
    for M in (A, R, D):
        spmv.csr_destroy(M)


def test_setup_apply_and_solve_checks_before_any_device_work(spmv):
    E = spmv.SpMVError
    A = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    R = spmv.csr_wrap_device(8, 6, 16, FAKE_RP, FAKE_CI, FAKE_VA)
    Z = spmv.csr_wrap_device(0, 0, 0, FAKE_RP, None, None)
    H = spmv.csr_from_arrays(2, 2, [0, 1, 2], [0, 1], np.ones(2, np.float32))    # host only
    NC = spmv.csr_wrap_device(8, 8, 16, FAKE_RP, None, FAKE_VA)
    lib = spmv.lib()
    out = spmv.AMGResult(error_code=7, levels=9)
    assert lib.spmv_c_amg_setup(None, A, None, 0, None, ctypes.byref(out)) == E.INVALID_ARGUMENT
    assert out.error_code == E.INVALID_ARGUMENT and (out.levels, out.bad_row, out.bad_level) == (0, -1, -1)
    handle = ctypes.c_void_p(0x1234)
    assert lib.spmv_c_amg_setup(ctypes.byref(handle), None, None, 0, None, None) == E.INVALID_ARGUMENT
    assert handle.value is None                                                  # *out is null on failure
    bad_cfg = spmv.AMGConfig(max_levels=0)
    for M, cfg, code in ((R, bad_cfg, E.INVALID_DIMENSION), (Z, bad_cfg, E.INVALID_DIMENSION),
                         (H, bad_cfg, E.INVALID_FORMAT), (NC, bad_cfg, E.INVALID_FORMAT)):
        res, handle = spmv.amg_setup(M, cfg)
        assert res.error_code == code and handle is None
    for field, value in (("max_levels", 0), ("coarse_rows", 0), ("coarse_rows", 1025), ("strength", -0.1),
                         ("strength", float("nan")), ("pre_sweeps", 0), ("post_sweeps", -1), ("jacobi_weight", 0.0),
                         ("jacobi_weight", 2.0), ("jacobi_weight", float("nan")), ("coarse_sweeps", 0)):
        res, handle = spmv.amg_setup(A, spmv.AMGConfig(**{field: value}))
        assert res.error_code == E.INVALID_ARGUMENT and handle is None, (field, value)
    # caller-given aggregates: out of range, an aggregate without members, a second map sized by the first
    good = np.array([0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    for maps in ([np.array([0, 0, 1, 1, 2, 2, 3, 8], np.int32)], [np.array([0, 0, 1, 1, 2, 2, -1, 3], np.int32)],
                 [np.array([0, 0, 1, 1, 3, 3, 4, 4], np.int32)], [good, np.array([0, 0, 1, 4], np.int32)],
                 [good, np.array([0, 0, 2, 2], np.int32)]):
        res, handle = spmv.amg_setup(A, None, maps)
        assert res.error_code == E.INVALID_ARGUMENT and handle is None, maps
    table = (ctypes.c_void_p * 1)(None)
    assert lib.spmv_c_amg_setup(ctypes.byref(ctypes.c_void_p()), A, None, 1, table, None) == E.INVALID_ARGUMENT
    assert lib.spmv_c_amg_setup(ctypes.byref(ctypes.c_void_p()), A, None, -1, table, None) == E.INVALID_ARGUMENT
    # null hierarchies
    assert spmv.amg_num_levels(None) == 0
    spmv.amg_destroy(None)
    assert spmv.amg_apply(None, 0x1000, 0x2000) == E.INVALID_ARGUMENT
    assert spmv.amg_update(None, A).error_code == E.INVALID_ARGUMENT
    assert spmv.amg_level(None, 0)[0] == E.INVALID_ARGUMENT
    # cg_solve_amg: cg_solve's checks first, then the null hierarchy
    assert spmv.cg_solve_amg(A, None, None, 0x2000).error_code == E.INVALID_ARGUMENT
    assert spmv.cg_solve_amg(R, None, 0x1000, 0x2000).error_code == E.INVALID_DIMENSION
    assert spmv.cg_solve_amg(H, None, 0x1000, 0x2000).error_code == E.INVALID_FORMAT
    assert spmv.cg_solve_amg(A, None, 0x1000, 0x2000, spmv.CGConfig(tolerance=-1.0)).error_code == E.INVALID_ARGUMENT
    assert spmv.cg_solve_amg(A, None, 0x1000, 0x1004).error_code == E.INVALID_ARGUMENT       # overlap
    assert spmv.cg_solve_amg(A, None, 0x1000, 0x2000).error_code == E.INVALID_ARGUMENT       # null H
    assert spmv.cg_solve_amg(Z, None, 0x1000, 0x2000).error_code == 0                        # no rows: nothing to do
    for M in (A, R, Z, H, NC):
        spmv.csr_destroy(M)


# ---- the sanitized caller --------------------------------------------------------------------------------------
def test_amg_host_is_clean_under_asan_and_ubsan():
    """make -C gpu-spmv_amd sanitize-amg builds tests/cpp/bin/amg_host_sanitized (csrc/amg_host.cpp and
    tests/cpp/amg_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    built = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-amg"], capture_output=True,
                           text=True)
    assert built.returncode == 0, built.stdout[-2000:] + built.stderr[-2000:]
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "amg_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
