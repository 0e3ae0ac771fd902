"""fsai_csr / fsai_csr_numeric (include/spmv/fsai.h) on the GPU: the device G against fsai_cpu_csr with np.array_equal
on values, columns and row pointers, at every forced lane count and row class, at each class edge, on sizes that leave the
last wavefront and workgroup partial, on rows of length 1 and 64 in one wavefront, on patterns sparser and richer than
A; the exact tier against the Fraction inverse; the rejections with G untouched; the refill; the reported bad row."""
import functools
import importlib

import numpy as np
import pytest

import fsai_cases as fc
import ic0_cases
from test_fsai_host import bits, host_fsai, rejected

pytestmark = pytest.mark.gpu

LANES = (1, 2, 4, 8, 16, 32, 64)
spd = importlib.import_module("gpu-spmv_amd.spd")


def _with_pattern(matrix, make_pattern):
    n, rp, ci, va = matrix
    return n, rp, ci, va, make_pattern(n, rp, ci)


# name -> (n, rp, ci, va, pattern or None)
SHAPES = {
    "n=1": lambda: (1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0], np.float32), None),
    "dense_spd_block(64)": lambda: fc.dense_spd_block(64) + (None,),
    # m = b + 1 at each class edge
    "banded_spd(150,3) m=4": lambda: fc.banded_spd(150, 3) + (None,),
    "banded_spd(150,4) m=5": lambda: fc.banded_spd(150, 4) + (None,),
    "banded_spd(150,7) m=8": lambda: fc.banded_spd(150, 7) + (None,),
    "banded_spd(150,8) m=9": lambda: fc.banded_spd(150, 8) + (None,),
    "banded_spd(150,15) m=16": lambda: fc.banded_spd(150, 15) + (None,),
    "banded_spd(150,16) m=17": lambda: fc.banded_spd(150, 16) + (None,),
    "banded_spd(150,31) m=32": lambda: fc.banded_spd(150, 31) + (None,),
    "banded_spd(150,32) m=33": lambda: fc.banded_spd(150, 32) + (None,),
    "banded_spd(150,63) m=64": lambda: fc.banded_spd(150, 63) + (None,),
    # the last wavefront and workgroup partial (64 rows per workgroup at class 4 with 4 lanes, 256 with 1 lane)
    "banded_spd(63,2)": lambda: fc.banded_spd(63, 2) + (None,),
    "banded_spd(64,2)": lambda: fc.banded_spd(64, 2) + (None,),
    "banded_spd(65,2)": lambda: fc.banded_spd(65, 2) + (None,),
    "banded_spd(257,2)": lambda: fc.banded_spd(257, 2) + (None,),
    "mixed_rows: lengths 1 and 64": lambda: fc.mixed_rows() + (None,),
    "sorted_random_spd(2000,8)": lambda: ic0_cases.sorted_random_spd(2000, 8, 11) + (None,),
    "poisson2d(24)": lambda: spd.poisson2d(24) + (None,),
    "poisson3d(8)": lambda: spd.poisson3d(8) + (None,),
    "poisson2d(24), S = I": lambda: _with_pattern(spd.poisson2d(24), lambda n, rp, ci: fc.identity_pattern(n)),
    "banded_spd(150,8), S = its band of 2": lambda: _with_pattern(fc.banded_spd(150, 8),
                                                                 lambda n, rp, ci: fc.band_of(n, rp, ci, 2)),
    "poisson2d(24), S = A*A": lambda: _with_pattern(spd.poisson2d(24), fc.squared_pattern),
    "poisson3d(8), S = A*A": lambda: _with_pattern(spd.poisson3d(8), fc.squared_pattern),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the shape and fsai_cpu_csr's G for it, computed once and never written to"""
    spmv = importlib.import_module("gpu-spmv_amd")
    n, rp, ci, va, pattern = SHAPES[name]()
    status, bad, want = host_fsai(spmv, n, rp, ci, va, pattern)
    assert (status, bad) == (0, -1)
    for a in want:
        a.setflags(write=False)
    return (n, rp, ci, va, pattern), want


def _upload(gpu, n, rp, ci, va):
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    return A


def _upload_pattern(gpu, n, pattern):
    return None if pattern is None else _upload(gpu, n, pattern[0], pattern[1], np.zeros(len(pattern[1]), np.float32))


def _read(gpu, G):
    assert gpu.csr_from_gpu(G) == 0
    return gpu.csr_host_arrays(G)


def _expected_lanes(max_row):
    lanes = 1
    while lanes < max_row:
        lanes *= 2
    return lanes


def _check_equal(got, want, tag):
    for g, w, what in zip(got, want, ("row_ptrs", "col_indices", "values")):
        if what == "values":
            assert np.array_equal(bits(g), bits(w)), (tag, what)
        else:
            assert np.array_equal(g, w), (tag, what)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_g_equals_the_cpu_bit_for_bit(gpu, monkeypatch, name):
    (n, rp, ci, va, pattern), want = reference(name)
    max_row = int(np.diff(want[0]).max())
    A, S = _upload(gpu, n, rp, ci, va), _upload_pattern(gpu, n, pattern)
    G = gpu.csr_create(1, 1, 0)
    try:
        for forced in (None, "fsai_lanes=1", "fsai_lanes=64", f"fsai_lanes=2,fsai_class={fc.class_for(max_row)}"):
            if forced is None:
                monkeypatch.delenv("SPMV_DEBUG", raising=False)
            else:
                monkeypatch.setenv("SPMV_DEBUG", forced)
            res = gpu.fsai_csr(G, A, S)
            tag = f"{name} {forced}"
            assert (res.error_code, res.bad_row, res.long_row) == (0, -1, -1), tag
            assert (res.nnz, res.max_row, res.row_class) == (want[1].size, max_row, fc.class_for(max_row)), tag
            lanes = _expected_lanes(max_row) if forced is None else int(forced.split(",")[0].split("=")[1])
            assert res.lanes_per_row == lanes and res.elapsed_ms > 0, tag
            m = G.contents
            assert (m.num_rows, m.num_cols, m.nnz) == (n, n, want[1].size) and m.owns_device_memory, tag
            _check_equal(_read(gpu, G), want, tag)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        for M in (A, S, G):
            gpu.csr_destroy(M)


@pytest.mark.parametrize("lanes", LANES)
def test_dense_block_of_64_at_every_forced_lane_count(gpu, monkeypatch, lanes):
    (n, rp, ci, va, _), want = reference("dense_spd_block(64)")
    A = _upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    try:
        monkeypatch.setenv("SPMV_DEBUG", f"fsai_lanes={lanes},fsai_class=64")
        res = gpu.fsai_csr(G, A)
        assert (res.error_code, res.max_row, res.row_class, res.lanes_per_row) == (0, 64, 64, lanes)
        _check_equal(_read(gpu, G), want, f"lanes={lanes}")
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(G)


@pytest.mark.parametrize("row_class", fc.CLASSES)
def test_every_class_at_every_lane_count_gives_the_same_bits(gpu, monkeypatch, row_class):
    """rows of at most 3 entries fit every class; 257 rows leave the last workgroup partial in each"""
    (n, rp, ci, va, _), want = reference("banded_spd(257,2)")
    A = _upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    try:
        for lanes in LANES:
            monkeypatch.setenv("SPMV_DEBUG", f"fsai_lanes={lanes},fsai_class={row_class}")
            res = gpu.fsai_csr(G, A)
            assert (res.error_code, res.max_row, res.row_class, res.lanes_per_row) == (0, 3, row_class, lanes)
            _check_equal(_read(gpu, G), want, f"class={row_class} lanes={lanes}")
        # a value that is no class or no lane count is ignored
        monkeypatch.setenv("SPMV_DEBUG", "fsai_lanes=3,fsai_class=12")
        res = gpu.fsai_csr(G, A)
        assert (res.error_code, res.row_class, res.lanes_per_row) == (0, 4, 4)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(G)


def test_a_forced_class_below_the_longest_row_is_rejected(gpu, monkeypatch):
    (n, rp, ci, va, _), want = reference("banded_spd(150,8) m=9")
    A = _upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    try:
        monkeypatch.setenv("SPMV_DEBUG", "fsai_class=8")
        res = gpu.fsai_csr(G, A)
        assert res.error_code == gpu.SpMVError.INVALID_ARGUMENT and res.max_row == 9 and res.long_row == -1
        assert (G.contents.num_rows, G.contents.nnz) == (1, 0) and not G.contents.d_row_ptrs
        monkeypatch.setenv("SPMV_DEBUG", "fsai_class=32")
        res = gpu.fsai_csr(G, A)
        assert (res.error_code, res.row_class) == (0, 32)
        monkeypatch.setenv("SPMV_DEBUG", "fsai_class=8")
        assert gpu.fsai_csr_numeric(G, A).error_code == gpu.SpMVError.INVALID_ARGUMENT
        _check_equal(_read(gpu, G), want, "after the rejected refill")
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
        gpu.csr_destroy(A)
        gpu.csr_destroy(G)


@pytest.mark.parametrize("sizes", [(1, 2, 3, 4, 5, 6), (6, 6, 5, 1, 6) * 3])
def test_the_exact_tier_at_zero_tolerance(gpu, sizes):
    n, rp, ci, va, L = fc.exact_blocks(sizes)
    want = fc.prove_exact(n, rp, ci, va, L)
    A = _upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    res = gpu.fsai_csr(G, A)
    assert (res.error_code, res.bad_row, res.max_row, res.row_class) == (0, -1, 6, 8)
    g_rp, g_ci, g = _read(gpu, G)
    assert np.array_equal(bits(g), bits(want))
    dense = np.zeros((n, n))
    dense[fc.rows_of(n, g_rp), g_ci] = g
    assert np.array_equal(dense @ L, np.eye(n))
    gpu.csr_destroy(A)
    gpu.csr_destroy(G)


def _untouched(gpu, G, want):
    m = G.contents
    assert (m.num_rows, m.num_cols, m.nnz) == (want[0].size - 1, want[0].size - 1, want[1].size)
    _check_equal(_read(gpu, G), want, "G after a rejected call")


def test_rejections_leave_g_untouched(gpu):
    E = gpu.SpMVError
    (n, rp, ci, va, _), want = reference("banded_spd(63,2)")
    good = _upload(gpu, n, rp, ci, va)
    G = gpu.csr_create(1, 1, 0)
    assert gpu.fsai_csr(G, good).error_code == 0            # a G that holds something
    # a pattern row of 65 entries: the lowest such row is reported
    A = _upload(gpu, *fc.dense_spd_block(65))
    res = gpu.fsai_csr(G, A)
    assert (res.error_code, res.long_row, res.max_row) == (E.INVALID_ARGUMENT, 64, 65)
    _untouched(gpu, G, want)
    n2, rp2, ci2, va2 = fc.banded_spd(300, 70)
    B = _upload(gpu, n2, rp2, ci2, va2)
    res = gpu.fsai_csr(G, B)
    assert (res.error_code, res.long_row, res.max_row) == (E.INVALID_ARGUMENT, 64, 71)
    _untouched(gpu, G, want)
    gpu.csr_destroy(A)
    gpu.csr_destroy(B)
    # each device-side rejection of A and S
    for name, (matrix, pattern, code) in rejected().items():
        A = _upload(gpu, *matrix)
        S = _upload_pattern(gpu, matrix[0], pattern)
        res = gpu.fsai_csr(G, A, S)
        assert res.error_code == getattr(E, code), name
        _untouched(gpu, G, want)
        gpu.csr_destroy(A)
        gpu.csr_destroy(S)
    # aliases and shapes with real device arrays
    assert gpu.fsai_csr(good, good).error_code == E.INVALID_ARGUMENT
    assert gpu.fsai_csr(G, good, G).error_code == E.INVALID_ARGUMENT
    R = gpu.csr_from_arrays(2, 3, [0, 1, 2], [0, 1], np.asarray([4, 4], np.float32))
    assert gpu.csr_to_gpu(R) == 0
    assert gpu.fsai_csr(G, R).error_code == E.INVALID_DIMENSION
    assert gpu.fsai_csr(G, good, R).error_code == E.INVALID_DIMENSION
    assert gpu.fsai_csr_numeric(G, R).error_code == E.INVALID_DIMENSION
    _untouched(gpu, G, want)
    # no rows: an empty G
    Z = gpu.csr_create(0, 0, 0)
    res = gpu.fsai_csr(G, Z)
    assert (res.error_code, res.nnz, res.bad_row) == (0, 0, -1)
    assert (G.contents.num_rows, G.contents.nnz) == (0, 0) and G.contents.d_row_ptrs
    for M in (good, G, R, Z):
        gpu.csr_destroy(M)


def test_numeric_refill_equals_a_fresh_build(gpu):
    for name in ("sorted_random_spd(2000,8)", "poisson2d(24), S = A*A", "mixed_rows: lengths 1 and 64"):
        (n, rp, ci, va, pattern), want = reference(name)
        A, S = _upload(gpu, n, rp, ci, va), _upload_pattern(gpu, n, pattern)
        G = gpu.csr_create(1, 1, 0)
        first = gpu.fsai_csr(G, A, S)
        assert first.error_code == 0
        # new values on the same pattern: symmetric scaling keeps the matrix SPD
        scale = (1.0 + 0.25 * np.sin(np.arange(n))).astype(np.float32)
        new_va = (va * scale[fc.rows_of(n, rp)] * scale[ci]).astype(np.float32)
        A2 = _upload(gpu, n, rp, ci, new_va)
        fresh = gpu.csr_create(1, 1, 0)
        assert gpu.fsai_csr(fresh, A2, S).error_code == 0
        want2 = _read(gpu, fresh)
        _, _, host2 = host_fsai(gpu, n, rp, ci, new_va, pattern)
        _check_equal(want2, host2, name)
        assert not np.array_equal(bits(want2[2]), bits(want[2]))
        for turn in range(2):                    # twice in a row: the same bits
            res = gpu.fsai_csr_numeric(G, A2)
            assert (res.error_code, res.bad_row, res.nnz) == (0, -1, first.nnz), name
            assert (res.max_row, res.row_class, res.lanes_per_row) == (first.max_row, first.row_class,
                                                                       first.lanes_per_row), name
            _check_equal(_read(gpu, G), want2, f"{name} turn {turn}")
        assert gpu.fsai_csr_numeric(G, A).error_code == 0           # and back
        _check_equal(_read(gpu, G), want, name)
        # a G that fsai_csr did not build: the host's pattern, uploaded
        foreign = _upload(gpu, n, want[0], want[1], np.full(want[1].size, np.nan, np.float32))
        res = gpu.fsai_csr_numeric(foreign, A2)
        assert (res.error_code, res.max_row, res.row_class) == (0, first.max_row, first.row_class), name
        _check_equal(_read(gpu, foreign), want2, f"{name} foreign")
        for M in (A, S, G, A2, fresh, foreign):
            gpu.csr_destroy(M)


def test_bad_row_is_reported_like_the_cpu(gpu, monkeypatch):
    systems = {"indefinite(40,17)": fc.indefinite(40, 17)}
    n, rp, ci, va = spd.poisson3d(8)
    va = va.copy()
    r = fc.rows_of(n, rp)
    for row in (400, 130, 300):                  # the lowest bad row wins whatever order the scan meets them in
        va[(r == row) & (ci == row)] = -6.0
    systems["poisson3d(8), rows 130, 300, 400"] = (n, rp, ci, va)
    try:
        for name, (n, rp, ci, va) in systems.items():
            status, host_bad, want = host_fsai(gpu, n, rp, ci, va)
            assert status == 0 and host_bad == (17 if name.startswith("indefinite") else 130)
            A = _upload(gpu, n, rp, ci, va)
            G = gpu.csr_create(1, 1, 0)
            for lanes in (1, 8, None):
                if lanes is None:
                    monkeypatch.delenv("SPMV_DEBUG", raising=False)
                else:
                    monkeypatch.setenv("SPMV_DEBUG", f"fsai_lanes={lanes}")
                res = gpu.fsai_csr(G, A)
                assert (res.error_code, res.bad_row) == (0, host_bad), (name, lanes)
                got = _read(gpu, G)
                assert np.array_equal(np.isnan(got[2]), np.isnan(want[2])), name
                ok = ~np.isnan(want[2])
                assert np.array_equal(bits(got[2])[ok], bits(want[2])[ok]), name
                assert gpu.fsai_csr_numeric(G, A).bad_row == host_bad, name
            gpu.csr_destroy(A)
            gpu.csr_destroy(G)
    finally:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
