"""Multicolour reordering (include/spmv/reorder.h) on the host side (no GPU): the exported names and struct layouts;
csr_color_cpu and csr_permute_cpu against the restatement of the header in tests/reorder_cases.py at zero tolerance;
properness; colour(v) == v's LOWER level in P A P^T, hence num_levels == num_colors for both triangles; fmix32 against
hand-computed values; the colour counts recorded in tests/golden/reorder_restate.json against a fresh run; the argument
checks that come before any device work; and csrc/reorder_host.cpp under AddressSanitizer + UBSan through a
stand-alone caller."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import reorder_cases as rc
from conftest import ROOT

COL, PERM, INV = 0x800000, 0x900000, 0xA00000          # fake, never-dereferenced device addresses
FAKE_RP, FAKE_CI, FAKE_VA = 0x500000, 0x600000, 0x700000

ALL = dict(rc.SMALL)
ALL.update(rc.LIBRARY)
ALL.update({"K65": lambda: rc.complete(65), "star(300)": lambda: rc.star(300), "path(257)": lambda: rc.path(257)})


def test_names_exist_in_the_c_abi_the_library_and_python(spmv):
    names = ("csr_color", "csr_color_cpu", "color_ordering", "csr_permute_gpu", "csr_permute_cpu", "permute_gather",
             "permute_gather_async", "multicolor_reorder")
    header = open(os.path.join(ROOT, "include", "spmv_c.h")).read()
    for name in names:
        assert "spmv_c_" + name in spmv.EXPORTED_SYMBOLS and hasattr(spmv.lib(), "spmv_c_" + name)
        assert "spmv_c_" + name + "(" in header and callable(getattr(spmv, name))
    public = open(os.path.join(ROOT, "include", "spmv", "reorder.h")).read()
    for name in names:
        assert " " + name + "(" in public


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R = spmv.ColorConfig, spmv.ColorResult
    assert ctypes.sizeof(C) == 16 and ctypes.sizeof(R) == 20
    assert [f for f, _ in C._fields_] == ["seed", "symmetric_pattern", "lanes_per_row", "reserved"]
    assert [f for f, _ in R._fields_] == ["error_code", "num_colors", "rounds", "launches", "elapsed_ms"]
    assert [getattr(C, f).offset for f, _ in C._fields_] == [0, 4, 8, 12]
    assert [getattr(R, f).offset for f, _ in R._fields_] == [0, 4, 8, 12, 16]
    c = C()
    assert (c.seed, c.symmetric_pattern, c.lanes_per_row, c.reserved) == (0, 0, 0, 0)
    assert C(seed=0xFFFFFFFF).seed == 0xFFFFFFFF


def test_fmix32_against_hand_computed_values():
    """0 is a fixed point.  For 1, step by step in 32-bit arithmetic: 1 ^ (1 >> 16) = 1; * 0x85ebca6b = 0x85ebca6b;
    ^ (>> 13 = 0x00042f5e) = 0x85efe535; * 0xc2b2ae35 = 0x514e79f9 (mod 2^32); ^ (>> 16 = 0x514e) = 0x514e28b7."""
    assert rc.fmix32(0) == 0
    assert rc.fmix32(1) == 0x514E28B7
    assert rc.fmix32(2) == 0x30F4C306
    assert rc.fmix32(0xFFFFFFFF) == 0x81F16F39
    assert rc.fmix32(12345) == 0x3C46C9DC
    # a bijection: no two of the first 4096 integers collide, so the index never breaks a tie
    assert len({rc.fmix32(i) for i in range(4096)}) == 4096
    assert rc.priority(1) > rc.priority(2) and rc.priority(5, seed=5) == (0, 5)


@pytest.mark.parametrize("name", list(ALL))
def test_csr_color_cpu_is_the_restatement(spmv, name):
    n, rp, ci, va = ALL[name]()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    for seed in (0, 1, 0xDEADBEEF):
        for promised in (0, 1):
            want, want_colors, want_rounds = rc.color(n, rp, ci, seed, promised)
            status, got, colors, rounds = spmv.csr_color_cpu(A, spmv.ColorConfig(seed=seed, symmetric_pattern=promised))
            assert status == 0
            assert np.array_equal(got, want), (name, seed, promised)
            assert (colors, rounds) == (want_colors, want_rounds), (name, seed, promised)
            if not promised:
                assert rc.is_proper(n, rp, ci, got), (name, seed)
    # the synchronous Jones-Plassmann iteration arrives at the same colours in the number of rounds reported
    if n <= 600:
        by_rounds, colors, rounds = rc.color_by_rounds(n, rp, ci)
        status, got, got_colors, got_rounds = spmv.csr_color_cpu(A)
        assert np.array_equal(got, by_rounds) and (got_colors, got_rounds) == (colors, rounds)
    spmv.csr_destroy(A)


def test_a_broken_symmetry_promise_gives_a_defined_improper_colouring(spmv):
    n, rp, ci, va = rc.upper_bidiagonal(40)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, honest, colors, _ = spmv.csr_color_cpu(A)
    assert status == 0 and rc.is_proper(n, rp, ci, honest) and colors in (2, 3)
    status, promised, _, _ = spmv.csr_color_cpu(A, spmv.ColorConfig(symmetric_pattern=1))
    assert status == 0 and np.array_equal(promised, rc.color(n, rp, ci, 0, 1)[0])
    assert not rc.is_proper(n, rp, ci, promised)          # vertex i never looks at i - 1
    spmv.csr_destroy(A)


# A level schedule reads the STORED pattern of one triangle, a colouring the symmetrised graph: the two coincide where
# the pattern is structurally symmetric, which IC(0) demands and every grid and SPD generator of the library gives.
SYMMETRIC = [name for name in ALL if rc.structurally_symmetric(*ALL[name]()[:3])]


@pytest.mark.parametrize("name", SYMMETRIC)
def test_a_colour_is_the_level_in_the_permuted_matrix(spmv, name):
    n, rp, ci, va = ALL[name]()
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, colors, num_colors, _ = spmv.csr_color_cpu(A)
    assert status == 0
    perm, inverse, color_ptr = rc.ordering(colors, num_colors)
    B = spmv.csr_create(0, 0, 0)
    assert spmv.csr_permute_cpu(B, A, perm, inverse) == 0
    b_rp, b_ci, b_va = spmv.csr_host_arrays(B)
    want = rc.permute(n, n, rp, ci, va, perm, inverse)
    assert np.array_equal(b_rp, want[0]) and np.array_equal(b_ci, want[1])
    assert np.array_equal(b_va.view(np.uint32), want[2].view(np.uint32))
    status, level_ptr, order, levels, _ = spmv.sptrsv_levels(n, b_rp, b_ci, 0)
    assert status == 0 and levels == num_colors and np.array_equal(level_ptr, color_ptr)
    assert np.array_equal(order, np.arange(n))            # new index order IS (level, row) order
    level_of = np.repeat(np.arange(levels), np.diff(level_ptr))
    assert np.array_equal(level_of[inverse], colors)      # colour(v) == LOWER level of v's new row
    assert spmv.sptrsv_levels(n, b_rp, b_ci, 1)[3] == num_colors
    spmv.csr_destroy(A)
    spmv.csr_destroy(B)


def test_recorded_colour_counts_against_a_fresh_run(spmv):
    with open(os.path.join(ROOT, "tests", "golden", rc.GOLDEN)) as f:
        recorded = json.load(f)
    assert set(recorded) == set(rc.COUNTED)
    for name, make in rc.COUNTED.items():
        n, rp, ci, va = make()
        colors, num_colors, rounds = rc.color(n, rp, ci)
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        status, got, got_colors, got_rounds = spmv.csr_color_cpu(A)
        spmv.csr_destroy(A)
        assert status == 0 and np.array_equal(got, colors)
        print(name, "colours", num_colors, "synchronous rounds", rounds)
        assert recorded[name] == {"num_colors": num_colors, "rounds": rounds} == {"num_colors": got_colors,
                                                                                 "rounds": got_rounds}
        assert num_colors == rc.QUOTED_COLORS[name]


PERMUTE_CASES = {
    "rectangular": lambda: rc.with_row_lengths([3, 0, 17, 1, 64, 5, 65, 9, 0, 33] * 3 + [7] * 7, 91, seed=1),
    "repeats": lambda: rc.with_row_lengths([0, 1, 5, 40, 130, 64, 63, 65, 2], 60, seed=2, repeats=True),
    "long": lambda: rc.with_row_lengths([5000, 3, 0, 700], 6000, seed=3),
}


@pytest.mark.parametrize("name", list(PERMUTE_CASES))
def test_csr_permute_cpu_is_the_restatement(spmv, name):
    rows, cols, rp, ci, va = PERMUTE_CASES[name]()
    A = spmv.csr_from_arrays(rows, cols, rp, ci, va)
    rng = np.random.default_rng(5)
    row_perm, col_inverse = rng.permutation(rows).astype(np.int32), rng.permutation(cols).astype(np.int32)
    for rperm, cinv in ((None, None), (row_perm, None), (None, col_inverse), (row_perm, col_inverse),
                        (np.arange(rows)[::-1], np.arange(cols)[::-1])):
        B = spmv.csr_create(2, 2, 1)
        assert spmv.csr_permute_cpu(B, A, rperm, cinv) == 0
        got = spmv.csr_host_arrays(B)
        want = rc.permute(rows, cols, rp, ci, va, rperm, cinv)
        assert (B.contents.num_rows, B.contents.num_cols, B.contents.nnz) == (rows, cols, ci.size)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        spmv.csr_destroy(B)
    spmv.csr_destroy(A)


def test_csr_permute_cpu_keeps_every_bit_pattern_and_comes_back(spmv):
    n, rp, ci, va = rc.messy()
    va = va.copy()
    va.view(np.uint32)[:4] = (0x80000000, 0x7FC00001, 0xFFC12345, 0x00000001)     # -0, two NaN payloads, a denormal
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    perm = np.random.default_rng(1).permutation(n).astype(np.int32)
    inverse = np.empty(n, np.int32)
    inverse[perm] = np.arange(n, dtype=np.int32)
    B, C, S = spmv.csr_create(0, 0, 0), spmv.csr_create(0, 0, 0), spmv.csr_create(0, 0, 0)
    assert spmv.csr_permute_cpu(B, A, perm, inverse) == 0          # P A P^T
    assert spmv.csr_permute_cpu(C, B, inverse, perm) == 0          # and back
    assert spmv.csr_permute_cpu(S, A, None, None) == 0             # A's sorted form
    back, sorted_form = spmv.csr_host_arrays(C), spmv.csr_host_arrays(S)
    assert np.array_equal(back[0], sorted_form[0]) and np.array_equal(back[1], sorted_form[1])
    assert np.array_equal(back[2].view(np.uint32), sorted_form[2].view(np.uint32))
    assert sorted(spmv.csr_host_arrays(B)[2].view(np.uint32).tolist()) == sorted(va.view(np.uint32).tolist())
    for M in (A, B, C, S):
        spmv.csr_destroy(M)


def test_host_rejections(spmv):
    E = spmv.SpMVError
    n, rp, ci, va = rc.path(6)
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    R = spmv.csr_create(3, 4, 0)
    Z = spmv.csr_create(0, 0, 0)
    assert spmv.csr_color_cpu(None)[0] == E.INVALID_ARGUMENT
    assert spmv.lib().spmv_c_csr_color_cpu(A, None, None, None, None) == E.INVALID_ARGUMENT
    assert spmv.csr_color_cpu(R)[0] == E.INVALID_DIMENSION
    assert spmv.csr_color_cpu(Z, spmv.ColorConfig(reserved=1))[:3:2] == (0, 0)
    for cfg in (spmv.ColorConfig(lanes_per_row=3), spmv.ColorConfig(lanes_per_row=128),
                spmv.ColorConfig(lanes_per_row=-2), spmv.ColorConfig(reserved=1)):
        assert spmv.csr_color_cpu(A, cfg)[0] == E.INVALID_ARGUMENT
    bad_ci = ci.copy()
    bad_ci[4] = n
    M = spmv.csr_from_arrays(n, n, rp, bad_ci, va)
    assert spmv.csr_color_cpu(M)[0] == E.INVALID_FORMAT
    B = spmv.csr_create(1, 1, 0)
    assert spmv.csr_permute_cpu(B, M) == E.INVALID_FORMAT
    assert spmv.csr_permute_cpu(B, A, [0, 1, 2, 3, 4, 4]) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_cpu(B, A, None, [0, 1, 2, 3, 4, 6]) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_cpu(B, A, [-1, 1, 2, 3, 4, 5]) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_cpu(A, A) == E.INVALID_ARGUMENT and spmv.csr_permute_cpu(None, A) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_cpu(B, None) == E.INVALID_ARGUMENT
    assert (B.contents.num_rows, B.contents.num_cols, B.contents.nnz) == (1, 1, 0)       # as it was
    for X in (A, R, Z, M, B):
        spmv.csr_destroy(X)


def test_device_entry_points_check_before_any_device_work(spmv):
    """every call below must return before it touches a (fake) device address"""
    E = spmv.SpMVError
    Cfg = spmv.ColorConfig
    bad = Cfg(lanes_per_row=3, reserved=9)
    D = spmv.csr_wrap_device(100, 100, 300, FAKE_RP, FAKE_CI, FAKE_VA)
    n, rp, ci, va = rc.path(6)
    H = spmv.csr_from_arrays(n, n, rp, ci, va)                                          # host only
    # csr_color: nulls, not square, no rows, device arrays, lanes, reserved
    assert spmv.csr_color(None, COL, bad).error_code == E.INVALID_ARGUMENT
    assert spmv.csr_color(D, None, bad).error_code == E.INVALID_ARGUMENT
    R = spmv.csr_wrap_device(5, 4, 0, FAKE_RP, FAKE_CI, FAKE_VA)
    assert spmv.csr_color(R, COL, bad).error_code == E.INVALID_DIMENSION
    Z = spmv.csr_create(0, 0, 0)
    res = spmv.csr_color(Z, COL, bad)
    assert (res.error_code, res.num_colors, res.rounds, res.launches) == (0, 0, 0, 0)
    assert spmv.csr_color(H, COL, bad).error_code == E.INVALID_FORMAT
    for rp_, ci_, va_ in ((FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
        M = spmv.csr_wrap_device(8, 8, 16, rp_, ci_, va_)
        assert spmv.csr_color(M, COL, bad).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(M)
    for cfg in (Cfg(lanes_per_row=3), Cfg(lanes_per_row=-1), Cfg(lanes_per_row=128), Cfg(reserved=1), bad):
        assert spmv.csr_color(D, COL, cfg).error_code == E.INVALID_ARGUMENT
    # multicolor_reorder: its own nulls and B == A, then csr_color's
    B = spmv.csr_create(0, 0, 0)
    assert spmv.multicolor_reorder(None, D, PERM, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.multicolor_reorder(B, None, PERM, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.multicolor_reorder(B, D, None, INV).error_code == E.INVALID_ARGUMENT
    assert spmv.multicolor_reorder(B, D, PERM, None).error_code == E.INVALID_ARGUMENT
    assert spmv.multicolor_reorder(D, D, PERM, INV).error_code == E.INVALID_ARGUMENT
    # color_ordering
    assert spmv.color_ordering(10, None, 3, PERM, INV)[0] == E.INVALID_ARGUMENT
    assert spmv.color_ordering(10, COL, 3, None, INV)[0] == E.INVALID_ARGUMENT
    assert spmv.color_ordering(10, COL, 3, PERM, None)[0] == E.INVALID_ARGUMENT
    assert spmv.color_ordering(-1, COL, 3, PERM, INV)[0] == E.INVALID_ARGUMENT
    assert spmv.color_ordering(10, COL, -1, PERM, INV)[0] == E.INVALID_ARGUMENT
    assert spmv.color_ordering(10, COL, 0, PERM, INV)[0] == E.INVALID_ARGUMENT
    status, color_ptr = spmv.color_ordering(0, COL, 2, PERM, INV)
    assert status == 0 and np.array_equal(color_ptr, [0, 0, 0])
    # csr_permute_gpu
    assert spmv.csr_permute_gpu(None, D) == E.INVALID_ARGUMENT and spmv.csr_permute_gpu(B, None) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_gpu(D, D, PERM, INV) == E.INVALID_ARGUMENT
    assert spmv.csr_permute_gpu(B, H, PERM, INV) == E.INVALID_FORMAT
    assert (B.contents.num_rows, B.contents.nnz) == (0, 0)
    # permute_gather: n = 10, k = 3, ldo = 5, ldi = 4
    OUT, IN, IDX = 0x100000, 0x200000, 0x300000
    for call in (spmv.permute_gather, lambda *a, **kw: spmv.permute_gather_async(*a, stream=None, **kw)):
        assert call(None, IN, IDX, 10, 3) == E.INVALID_ARGUMENT and call(OUT, None, IDX, 10, 3) == E.INVALID_ARGUMENT
        assert call(OUT, IN, None, 10, 3) == E.INVALID_ARGUMENT and call(OUT, IN, IDX, -1, 3) == E.INVALID_ARGUMENT
        for k in (0, -1, 33):
            assert call(OUT, IN, IDX, 10, k, ldo=40, ldi=40) == E.INVALID_ARGUMENT
        assert call(OUT, IN, IDX, 10, 3, ldo=2, ldi=4) == E.INVALID_ARGUMENT
        assert call(OUT, IN, IDX, 10, 3, ldo=5, ldi=2) == E.INVALID_ARGUMENT
        assert call(OUT, OUT, IDX, 10, 3) == E.INVALID_ARGUMENT
        assert call(OUT, OUT + 4 * 47, IDX, 10, 3, ldo=5, ldi=4) == E.INVALID_ARGUMENT
        assert call(OUT, OUT - 4 * 38, IDX, 10, 3, ldo=5, ldi=4) == E.INVALID_ARGUMENT
        assert call(OUT, OUT, IDX, 0, 3) == 0                                           # nothing to do
    for X in (D, H, R, Z, B):
        spmv.csr_destroy(X)


def test_reorder_host_under_sanitizers():
    """make -C gpu-spmv_amd sanitize-reorder builds tests/cpp/bin/reorder_host_sanitized (csrc/reorder_host.cpp and
    tests/cpp/reorder_host_sanitized.cpp under AddressSanitizer + UBSan); any sanitizer report aborts it."""
    build = subprocess.run(["make", "-C", os.path.join(ROOT, "gpu-spmv_amd"), "sanitize-reorder"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    # leak checking off: the HIP runtime's own start-up allocations are not ours to free
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "bin", "reorder_host_sanitized")], capture_output=True,
                         text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "all checks passed" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
