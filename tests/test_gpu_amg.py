"""amg_setup / amg_update / amg_level / amg_apply (include/spmv/amg.h) on the device.

The hierarchy is checked at zero tolerance: every level matrix against spgemm_cpu_csr applied twice to the aggregates
read back, the aggregates against amg_aggregate_cpu_csr of the downloaded level, Poisson levels against integer
arithmetic, pair aggregates on tridiag(-1, 2, -1), and amg_update against a fresh setup.  The V-cycle is checked bit
for bit, at every lane count, where amg_cases' prover shows that nothing rounds; elsewhere against the fp64 numpy
cycle on the levels read back, within 8 x the distance between the fp32 and the fp64 restatement (never a figure
taken from the device)."""
import importlib

import numpy as np
import pytest

import amg_cases as ac
from amg_cases import bits

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
LANES = (1, 2, 4, 8, 16, 32, 64)


class Hier:
    """A matrix on the device with its hierarchy and two device vectors."""

    def __init__(self, gpu, n, rp, ci, va, cfg=None, maps=None):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, np.asarray(va, np.float32)
        self.cfg = cfg if cfg is not None else gpu.AMGConfig()
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        self.res, self.H = gpu.amg_setup(self.A, self.cfg, maps)
        self.d_r, self.d_z = gpu.CudaBuffer(n), gpu.CudaBuffer(n)

    def levels(self):
        out = []
        for l in range(self.gpu.amg_num_levels(self.H)):
            n, rp, ci, va, agg = self.gpu.amg_level_arrays(self.H, l)
            count = self.gpu.amg_level(self.H, l)[3]
            out.append(dict(n=n, rp=rp, ci=ci, va=va, agg=agg, count=count))
        return out

    def apply(self, r):
        self.d_r.copyFromHost(np.asarray(r, np.float32), self.n)
        self.d_z.copyFromHost(np.full(self.n, np.nan, np.float32), self.n)
        assert self.gpu.amg_apply(self.H, self.d_r, self.d_z) == 0
        return self.d_z.copyToHost(self.n)

    def reference(self, r, dtype):
        c = self.cfg
        return ac.vcycle(self.levels(), r, c.jacobi_weight, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps, dtype)

    def close(self):
        self.gpu.amg_destroy(self.H)
        self.gpu.csr_destroy(self.A)
        self.d_r.release()
        self.d_z.release()


def assert_levels_equal(got, want, what=""):
    assert [g["n"] for g in got] == [w["n"] for w in want], what
    for l, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g["rp"], w["rp"], err_msg=f"row_ptrs of level {l} {what}")
        np.testing.assert_array_equal(g["ci"], w["ci"], err_msg=f"cols of level {l} {what}")
        np.testing.assert_array_equal(bits(g["va"]), bits(w["va"]), err_msg=f"value bits of level {l} {what}")
        assert (g["agg"] is None) == (w["agg"] is None), (l, what)
        if g["agg"] is not None:
            np.testing.assert_array_equal(g["agg"], w["agg"], err_msg=f"aggregates of level {l} {what}")


MATRICES = {
    "poisson2d(16)": lambda: spd.poisson2d(16),
    "poisson2d(32)": lambda: spd.poisson2d(32),
    "poisson3d(8)": lambda: spd.poisson3d(8),
    "random_spd(300, 7)": lambda: spd.random_spd(300, 7),
}


# ------------------------------------------------------------------------------------------ the hierarchy, bit for bit
@pytest.mark.parametrize("name", list(MATRICES))
def test_levels_are_the_host_products_and_the_host_aggregation(gpu, name):
    n, rp, ci, va = MATRICES[name]()
    cfg = gpu.AMGConfig(coarse_rows=16) if name.startswith("random") else None
    h = Hier(gpu, n, rp, ci, va, cfg)
    try:
        assert h.res.error_code == 0 and h.H is not None and (h.res.bad_row, h.res.bad_level) == (-1, -1)
        levels = h.levels()
        assert h.res.levels == len(levels) >= 2 and h.res.coarse_solver == 0 and h.res.setup_ms > 0
        # level 0 is a view over A's own arrays
        view = gpu.amg_level(h.H, 0)[1]
        a = h.A.contents
        assert [ctypes_address(p) for p in (view.d_row_ptrs, view.d_col_indices, view.d_values)] == \
            [ctypes_address(p) for p in (a.d_row_ptrs, a.d_col_indices, a.d_values)]
        assert not view.owns_device_memory and not view.owns_host_memory
        for got, want in zip((levels[0]["rp"], levels[0]["ci"], bits(levels[0]["va"])), (rp, ci, bits(va))):
            np.testing.assert_array_equal(got, want)
        for l, level in enumerate(levels[:-1]):
            host = gpu.csr_from_arrays(level["n"], level["n"], level["rp"], level["ci"], level["va"])
            status, agg, count = gpu.amg_aggregate_cpu_csr(host, h.cfg.strength)
            gpu.csr_destroy(host)
            assert status == 0 and count == level["count"] == levels[l + 1]["n"], (name, l)
            np.testing.assert_array_equal(level["agg"], agg)
            product = ac.galerkin(gpu, level["n"], level["rp"], level["ci"], level["va"], agg, count)
            for got, want in zip((levels[l + 1]["rp"], levels[l + 1]["ci"]), product[:2]):
                np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(bits(levels[l + 1]["va"]), bits(product[2]))
        assert levels[-1]["agg"] is None and levels[-1]["count"] == 0
        # the whole restated hierarchy, and the complexities
        assert_levels_equal(levels, ac.hierarchy(gpu, n, rp, ci, va, h.cfg.strength, h.cfg.coarse_rows), name)
        assert h.res.grid_complexity == pytest.approx(sum(lv["n"] for lv in levels) / n)
        assert h.res.operator_complexity == pytest.approx(sum(lv["ci"].size for lv in levels) / ci.size)
        if not name.startswith("random"):       # integer arithmetic: P^T A P of the integer matrix, entry for entry
            for l, level in enumerate(levels[:-1]):
                dense = ac.dense_of(level).astype(np.int64)
                P = np.zeros((level["n"], level["count"]), np.int64)
                P[np.arange(level["n"]), level["agg"]] = 1
                want = P.T @ dense @ P
                nxt = levels[l + 1]
                got = np.zeros_like(want)
                got[ac.rows_of(nxt["n"], nxt["rp"]), nxt["ci"]] = nxt["va"].astype(np.int64)
                np.testing.assert_array_equal(got, want)
                assert np.array_equal(nxt["va"], np.rint(nxt["va"]))
    finally:
        h.close()


def ctypes_address(p):
    import ctypes
    return ctypes.cast(p, ctypes.c_void_p).value


def test_level_sizes_are_the_restatements(gpu):
    for make, want in ((lambda: spd.poisson2d(16), [256, 48]), (lambda: spd.poisson3d(8), [512, 72, 14])):
        h = Hier(gpu, *make())
        try:
            assert [lv["n"] for lv in h.levels()] == want == [lv["n"] for lv in ac.hierarchy(gpu, *make())]
        finally:
            h.close()
    # max_levels cuts the hierarchy short; a stall ends it
    h = Hier(gpu, *spd.poisson2d(32), cfg=gpu.AMGConfig(max_levels=2))
    try:
        assert h.res.error_code == 0 and [lv["n"] for lv in h.levels()] == [1024, 176]
    finally:
        h.close()


def test_pair_aggregates_halve_the_tridiagonal_matrix(gpu):
    n, rp, ci, va = ac.tridiagonal(56)
    h = Hier(gpu, n, rp, ci, va, maps=ac.pair_maps(56, 7))
    try:
        assert h.res.error_code == 0 and h.res.levels == 4
        levels = h.levels()
        assert [lv["n"] for lv in levels] == [56, 28, 14, 7]
        for lv in levels:
            want = ac.tridiagonal(lv["n"])
            for got, expected in zip((lv["rp"], lv["ci"], lv["va"]), want[1:]):
                np.testing.assert_array_equal(got, expected)
        for lv in levels[:-1]:
            np.testing.assert_array_equal(lv["agg"], np.arange(lv["n"]) // 2)
        # more maps than max_levels allows: the level count still stops the hierarchy
        short = Hier(gpu, n, rp, ci, va, cfg=gpu.AMGConfig(max_levels=3), maps=ac.pair_maps(56, 7))
        assert short.res.error_code == 0 and [lv["n"] for lv in short.levels()] == [56, 28, 14]
        short.close()
    finally:
        h.close()


def test_update_equals_a_fresh_setup_and_a_wrong_matrix_leaves_the_hierarchy_usable(gpu):
    n, rp, ci, va = spd.random_spd(300, 7)
    cfg = gpu.AMGConfig(coarse_rows=16)
    h = Hier(gpu, n, rp, ci, va, cfg)
    try:
        before = h.levels()
        maps = [lv["agg"] for lv in before[:-1]]
        r = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
        z_before = h.apply(r)
        # another nnz: rejected before anything changes
        m, rp2, ci2, va2 = spd.random_spd(300, 6)
        other = gpu.csr_from_arrays(m, m, rp2, ci2, va2)
        assert gpu.csr_to_gpu(other) == 0
        res = gpu.amg_update(h.H, other)
        assert res.error_code == gpu.SpMVError.INVALID_DIMENSION
        gpu.csr_destroy(other)
        assert_levels_equal(h.levels(), before, "after the rejected update")
        np.testing.assert_array_equal(bits(h.apply(r)), bits(z_before))
        # 2 A through another handle: the hierarchy of amg_setup(2 A, the same aggregates), bit for bit
        doubled = Hier(gpu, n, rp, ci, 2 * va, cfg, maps=maps)
        assert doubled.res.error_code == 0
        res = gpu.amg_update(h.H, doubled.A)
        assert res.error_code == 0 and res.levels == len(before) and res.coarse_solver == 0
        updated = h.levels()
        assert_levels_equal(updated, doubled.levels(), "update against setup")
        for lv, old in zip(updated, before):
            np.testing.assert_array_equal(bits(lv["va"]), bits(2 * old["va"]))
        np.testing.assert_array_equal(bits(h.apply(r)), bits(doubled.apply(r)))
        # the same pattern with a row's diagonal gone bad: reported with its level and row
        bad = va.copy()
        row7 = np.flatnonzero((ac.rows_of(n, rp) == 7) & (ci == 7))
        bad[row7] = -1.0
        B = gpu.csr_from_arrays(n, n, rp, ci, bad)
        assert gpu.csr_to_gpu(B) == 0
        res = gpu.amg_update(h.H, B)
        assert (res.error_code, res.bad_level, res.bad_row) == (gpu.SpMVError.INVALID_ARGUMENT, 0, 7)
        assert gpu.amg_update(h.H, doubled.A).error_code == 0
        np.testing.assert_array_equal(bits(h.apply(r)), bits(doubled.apply(r)))
        gpu.csr_destroy(B)
        doubled.close()
    finally:
        h.close()


def test_bad_diagonals_and_structures_are_reported(gpu):
    E = gpu.SpMVError
    n, rp, ci, va = spd.poisson2d(16)
    for value, row in ((0.0, 5), (-4.0, 200), (np.nan, 0), (np.inf, 255)):
        bad = va.copy()
        bad[np.flatnonzero((ac.rows_of(n, rp) == row) & (ci == row))] = value
        h = Hier(gpu, n, rp, ci, bad)
        assert h.H is None and (h.res.error_code, h.res.bad_level, h.res.bad_row) == (E.INVALID_ARGUMENT, 0, row)
        h.close()
    keep = ~((ac.rows_of(n, rp) == 9) & (ci == 9))                 # row 9 stores no diagonal
    rp2 = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(ac.rows_of(n, rp)[keep], minlength=n), out=rp2[1:])
    h = Hier(gpu, n, rp2, ci[keep], va[keep])
    assert h.H is None and (h.res.error_code, h.res.bad_level, h.res.bad_row) == (E.INVALID_ARGUMENT, 0, 9)
    h.close()
    wild = ci.copy()
    wild[11] = n + 5
    h = Hier(gpu, n, rp, wild, va)
    assert h.H is None and h.res.error_code == E.INVALID_FORMAT
    h.close()
    # an indefinite coarsest level: the Cholesky pivot names its row
    n3, rp3, ci3, va3 = ac.tridiagonal(3)
    h = Hier(gpu, n3, rp3, ci3, np.where(va3 < 0, np.float32(-3.0), va3))
    assert h.H is None and (h.res.error_code, h.res.bad_level) == (E.INVALID_ARGUMENT, 0) and h.res.bad_row in (1, 2)
    h.close()


# ------------------------------------------------------------------------------------------ the V-cycle, exact tier
def test_the_stored_inverse_of_the_tridiagonal_matrix_is_exact(gpu):
    """one level of 7 rows: the cycle is the dense solve, and on unit vectors it reads the stored inverse out"""
    n, rp, ci, va = ac.tridiagonal(7)
    h = Hier(gpu, n, rp, ci, va)
    try:
        assert h.res.error_code == 0 and h.res.levels == 1 and h.res.coarse_solver == 0
        for j in range(n):
            want = np.array([(min(i, j) + 1) * (n - max(i, j)) / 8.0 for i in range(n)], np.float32)
            np.testing.assert_array_equal(bits(h.apply(np.eye(n, dtype=np.float32)[j])), bits(want))
    finally:
        h.close()


EXACT = [(24, 3), (28, 7), (56, 7), (112, 7)]


def test_exact_cycles_at_every_lane_count(gpu, monkeypatch):
    """tridiag(-1, 2, -1), pair aggregates, omega = 1/2, integer r in [-8, 8]: every quantity is dyadic.  The prover
    decides which (n, sweeps) run; the three single-sweep cases up to n = 56 must be among them."""
    admitted = []
    for n, coarsest in EXACT:
        for sweeps in (1, 2):
            r = ac.exact_rhs(n)
            want, width = ac.prove_vcycle(n, coarsest, r, 0.5, sweeps)
            print(f"n = {n}, sweeps = {sweeps}: " + (f"{width} bits" if want is not None else f"not admitted ({width})"))
            if want is None:
                continue
            admitted.append((n, sweeps))
            cfg = gpu.AMGConfig(jacobi_weight=0.5, pre_sweeps=sweeps, post_sweeps=sweeps)
            h = Hier(gpu, *ac.tridiagonal(n), cfg=cfg, maps=ac.pair_maps(n, coarsest))
            try:
                assert h.res.error_code == 0 and h.levels()[-1]["n"] == coarsest
                for lanes in LANES:
                    monkeypatch.setenv("SPMV_DEBUG", f"amg_lanes={lanes}")
                    np.testing.assert_array_equal(bits(h.apply(r)), bits(want), err_msg=f"n {n} lanes {lanes}")
                monkeypatch.delenv("SPMV_DEBUG")
                np.testing.assert_array_equal(bits(h.apply(r)), bits(want), err_msg=f"n {n}, the library's lanes")
            finally:
                h.close()
    assert {(24, 1), (28, 1), (56, 1)} <= set(admitted), admitted


# ------------------------------------------------------------------------------------------ the V-cycle, by bound
def arrow(n, width):
    """tridiag(-1, 4, -1) plus a first row and column of `width` further entries -1/8: row 0 is longer than a wavefront"""
    dense = np.zeros((n, n), np.float32)
    idx = np.arange(n)
    dense[idx, idx] = 4.0
    dense[idx[:-1], idx[:-1] + 1] = dense[idx[:-1] + 1, idx[:-1]] = -1.0
    dense[0, 2:2 + width] = dense[2:2 + width, 0] = -0.125
    dense[0, 0] = 32.0
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return n, rp, cols.astype(np.int32), dense[rows, cols]


def one_by_one():
    return 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0], np.float32)


def big_aggregate_map(n, members):
    return [np.concatenate([np.zeros(members, np.int32), np.arange(1, n - members + 1, dtype=np.int32)])]


# name: (matrix, config keywords, maps, expected levels or None, expected coarse solver)
EDGES = {
    "an aggregate of 130 rows beside singletons": (lambda: spd.poisson2d(15), {}, lambda: big_aggregate_map(225, 130), 2, 0),
    "a row of 200 entries": (lambda: arrow(256, 198), {}, lambda: ac.pair_maps(256, 128), 2, 0),
    "n = 257": (lambda: ac.tridiagonal(257), {"coarse_rows": 16}, None, 4, 0),
    "n = 63": (lambda: spd.random_spd(63, 5, seed=2), {"coarse_rows": 8}, None, None, 0),
    "one level": (lambda: spd.random_spd(40, 3, seed=4), {}, None, 1, 0),
    "n = 1": (one_by_one, {}, None, 1, 0),
    "a Jacobi-solved coarsest level": (lambda: spd.random_spd(1500, 7), {"strength": 10.0}, None, 1, 1),
    "Jacobi coarsest level, one sweep": (lambda: spd.random_spd(1500, 7), {"strength": 10.0, "coarse_sweeps": 1}, None, 1, 1),
    "no post-sweeps": (lambda: spd.poisson2d(16), {"pre_sweeps": 2, "post_sweeps": 0}, None, 2, 0),
    "three sweeps each side": (lambda: spd.poisson3d(8), {"pre_sweeps": 3, "post_sweeps": 3}, None, 3, 0),
    "unsorted rows, repeated columns": (lambda: spd.random_spd(300, 7), {"coarse_rows": 16}, None, None, 0),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_cycle_within_the_distance_of_the_two_restatements(gpu, name):
    make, keywords, maps, want_levels, want_solver = EDGES[name]
    n, rp, ci, va = make()
    h = Hier(gpu, n, rp, ci, va, gpu.AMGConfig(**keywords), maps() if maps else None)
    try:
        assert h.res.error_code == 0 and h.res.coarse_solver == want_solver, (name, h.res.error_code)
        if want_levels is not None:
            assert h.res.levels == want_levels, (name, h.res.levels)
        else:
            assert h.res.levels >= 2, (name, h.res.levels)
        r = np.random.default_rng(11).uniform(-1, 1, n).astype(np.float32)
        z32, z64 = h.reference(r, np.float32), h.reference(r, np.float64)
        bound = ac.tolerance(z32, z64)
        z = h.apply(r)
        error = float(np.max(np.abs(z.astype(np.float64) - z64)))
        print(f"{name}: levels {[lv['n'] for lv in h.levels()]}, error {error:.3g}, bound {bound:.3g}, "
              f"|z| {np.abs(z64).max():.3g}")
        assert np.isfinite(z).all() and error <= bound, (name, error, bound)
        np.testing.assert_array_equal(bits(h.apply(r)), bits(z))            # two applications, the same bits
    finally:
        h.close()


def test_vectors_that_are_views_into_larger_buffers(gpu):
    n, rp, ci, va = spd.poisson2d(16)
    h = Hier(gpu, n, rp, ci, va)
    try:
        r = np.random.default_rng(12).uniform(-1, 1, n).astype(np.float32)
        want = h.apply(r)
        front, back = 3, 5                                        # odd offsets: no 16-byte alignment of the views
        d_in, d_out = gpu.CudaBuffer(front + n + back), gpu.CudaBuffer(front + n + back)
        padded = np.full(front + n + back, np.nan, np.float32)    # NaN padding: a read of it would poison the result
        padded[front:front + n] = r
        d_in.copyFromHost(padded, padded.size)
        marks = np.arange(front + n + back, dtype=np.float32) + 0.5
        d_out.copyFromHost(marks, marks.size)
        assert gpu.amg_apply(h.H, d_in.get() + 4 * front, d_out.get() + 4 * front) == 0
        got = d_out.copyToHost(marks.size)
        np.testing.assert_array_equal(bits(got[front:front + n]), bits(want))
        np.testing.assert_array_equal(bits(got[:front]), bits(marks[:front]))
        np.testing.assert_array_equal(bits(got[front + n:]), bits(marks[front + n:]))
        np.testing.assert_array_equal(bits(d_in.copyToHost(padded.size)), bits(padded))
        # overlapping vectors are rejected and nothing is written
        assert gpu.amg_apply(h.H, d_out.get(), d_out.get() + 4) == gpu.SpMVError.INVALID_ARGUMENT
        np.testing.assert_array_equal(bits(d_out.copyToHost(marks.size)), bits(got))
        d_in.release()
        d_out.release()
    finally:
        h.close()
