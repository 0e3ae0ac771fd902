"""amg_setup_smoothed / amg_setup_smoothed_device / amg_level_transfer / amg_restrict / amg_prolong / amg_update on
smoothed hierarchies (include/spmv/amg.h, "Smoothed aggregation") on the device.

The hierarchy is checked at zero tolerance against amg_smoothed_cases.hierarchy, the chain of host twins with theta
decaying per level: every level matrix, every P and P^T, the aggregate maps and both complexities, for the three
builders.  The two transfers are checked bit for bit at every lane count where amg_smoothed_cases' prover shows that
nothing rounds.  The cycle is checked against the fp64 numpy cycle on the levels read back, within 8 x the distance
between the fp32 and the fp64 restatement (amg_cases.tolerance; never a figure taken from the device).  That every
kernel of the cycle returns at once when `done` is set is checked where `done` can be set: in
tests/test_gpu_cg_amg_smoothed.py, through cg_solve_amg's steps past convergence."""
import ctypes
import importlib

import numpy as np
import pytest

import amg_cases as ac
import amg_smoothed_cases as sc
from amg_cases import bits

pytestmark = pytest.mark.gpu

spd = importlib.import_module("gpu-spmv_amd.spd")
LANES = (1, 2, 4, 8, 16, 32, 64)
SEED = 3


def view_arrays(gpu, view):
    """numpy copies of a device view: (row_ptrs, cols, vals)"""
    def down(ptr, count, dtype):
        host = np.empty(count, dtype)
        address = ctypes.cast(ptr, ctypes.c_void_p).value
        if count:
            assert gpu.lib().spmv_c_memcpy_d2h(host.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(address),
                                               host.nbytes) == 0
        return host
    return (down(view.d_row_ptrs, view.num_rows + 1, np.int32), down(view.d_col_indices, view.nnz, np.int32),
            down(view.d_values, view.nnz, np.float32))


class Smoothed:
    """A matrix on the device with its smoothed hierarchy (builder: "host", "maps" or "device") and two vectors."""

    def __init__(self, gpu, n, rp, ci, va, cfg=None, smoothing=None, maps=None, builder="host"):
        self.gpu, self.n, self.rp, self.ci, self.va = gpu, n, rp, ci, np.asarray(va, np.float32)
        self.cfg = cfg if cfg is not None else gpu.AMGConfig()
        self.smoothing = smoothing if smoothing is not None else gpu.AMGSmoothing()
        self.A = gpu.csr_from_arrays(n, n, rp, ci, va)
        assert gpu.csr_to_gpu(self.A) == 0
        if builder == "device":
            self.res, self.H = gpu.amg_setup_smoothed_device(self.A, self.cfg, self.smoothing, SEED)
        else:
            self.res, self.H = gpu.amg_setup_smoothed(self.A, self.cfg, self.smoothing, maps)
        self.d_r, self.d_z = gpu.CudaBuffer(n), gpu.CudaBuffer(n)

    def levels(self):
        out = []
        count = self.gpu.amg_num_levels(self.H)
        for l in range(count):
            n, rp, ci, va, agg = self.gpu.amg_level_arrays(self.H, l)
            level = dict(n=n, rp=rp, ci=ci, va=va, agg=agg, count=self.gpu.amg_level(self.H, l)[3], P=None, PT=None)
            if l + 1 < count:
                status, p_view, pt_view = self.gpu.amg_level_transfer(self.H, l)
                assert status == 0
                assert (p_view.num_rows, p_view.num_cols) == (n, level["count"]) == (pt_view.num_cols, pt_view.num_rows)
                level["P"], level["PT"] = view_arrays(self.gpu, p_view), view_arrays(self.gpu, pt_view)
            out.append(level)
        return out

    def apply(self, r):
        self.d_r.copyFromHost(np.asarray(r, np.float32), self.n)
        self.d_z.copyFromHost(np.full(self.n, np.nan, np.float32), self.n)
        assert self.gpu.amg_apply(self.H, self.d_r, self.d_z) == 0
        return self.d_z.copyToHost(self.n)

    def reference(self, r, dtype):
        c = self.cfg
        return sc.vcycle(self.levels(), r, c.jacobi_weight, c.pre_sweeps, c.post_sweeps, c.coarse_sweeps, dtype)

    def close(self):
        self.gpu.amg_destroy(self.H)
        self.gpu.csr_destroy(self.A)
        self.d_r.release()
        self.d_z.release()


def assert_csr_equal(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg="row_ptrs of " + what)
    np.testing.assert_array_equal(got[1], want[1], err_msg="cols of " + what)
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]), err_msg="value bits of " + what)


def assert_levels_equal(got, want, what=""):
    assert [g["n"] for g in got] == [w["n"] for w in want], what
    for l, (g, w) in enumerate(zip(got, want)):
        assert_csr_equal((g["rp"], g["ci"], g["va"]), (w["rp"], w["ci"], w["va"]), f"level {l} {what}")
        assert (g["agg"] is None) == (w["agg"] is None) and g["count"] == w["count"], (l, what)
        if g["agg"] is not None:
            np.testing.assert_array_equal(g["agg"], w["agg"], err_msg=f"aggregates of level {l} {what}")
            assert_csr_equal(g["P"], w["P"], f"P of level {l} {what}")
            assert_csr_equal(g["PT"], w["PT"], f"PT of level {l} {what}")


MATRICES = {
    "poisson2d(32)": (lambda: spd.poisson2d(32), 64),
    "poisson3d(12)": (lambda: spd.poisson3d(12), 64),
    "random_spd(500, 7, 3)": (lambda: spd.random_spd(500, 7, 3), 16),
}


@pytest.fixture(scope="module")
def restated(gpu):
    """the restated hierarchies, computed once: (matrix name, "host" or "device") -> levels"""
    built = {}

    def get(name, builder, decay=0.5):
        key = (name, builder, decay)
        if key not in built:
            make, coarse_rows = MATRICES[name]
            aggregate = sc.mis2_aggregate(gpu, SEED) if builder == "device" else None
            built[key] = sc.hierarchy(gpu, *make(), coarse_rows=coarse_rows, decay=decay, aggregate=aggregate)
        return built[key]
    return get


# ------------------------------------------------------------------------------------------ the hierarchy, bit for bit
@pytest.mark.parametrize("builder", ["host", "maps", "device"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_levels_and_transfers_are_the_chain_of_host_twins(gpu, restated, name, builder):
    make, coarse_rows = MATRICES[name]
    n, rp, ci, va = make()
    want = restated(name, "device" if builder == "device" else "host")
    maps = [lv["agg"] for lv in want[:-1]] if builder == "maps" else None
    h = Smoothed(gpu, n, rp, ci, va, gpu.AMGConfig(coarse_rows=coarse_rows), maps=maps, builder=builder)
    try:
        assert h.res.error_code == 0 and h.H is not None and (h.res.bad_row, h.res.bad_level) == (-1, -1)
        assert gpu.amg_is_smoothed(h.H) == 1
        levels = h.levels()
        print(name, builder, "levels", [lv["n"] for lv in levels], "entries", [lv["ci"].size for lv in levels],
              "complexities %.3f %.3f" % (h.res.grid_complexity, h.res.operator_complexity))
        assert h.res.levels == len(levels) >= 3 and h.res.coarse_solver == 0 and h.res.setup_ms > 0
        assert_levels_equal(levels, want, f"{name} {builder}")
        assert h.res.grid_complexity == pytest.approx(sum(lv["n"] for lv in want) / n)
        assert h.res.operator_complexity == pytest.approx(sum(lv["ci"].size for lv in want) / ci.size)
        for l, level in enumerate(levels[:-1]):
            # amg_level's map is the aggregate map, not P's columns: n_l ints in [0, n_{l+1})
            assert level["agg"].shape == (level["n"],) and level["agg"].max() + 1 == level["count"] == levels[l + 1]["n"]
            assert level["P"][1].size > level["n"] or level["n"] == level["count"]
            # P^T is the stable transpose of P
            assert_csr_equal(level["PT"], sc.transpose(level["n"], level["count"], *level["P"]), f"PT of level {l}")
        assert gpu.amg_level_transfer(h.H, len(levels) - 1)[0] == gpu.SpMVError.INVALID_DIMENSION
        assert gpu.amg_level_transfer(h.H, -1)[0] == gpu.SpMVError.INVALID_DIMENSION
    finally:
        h.close()


def test_theta_decays_per_level(gpu, restated):
    """strength_decay = 1 keeps theta = 0.08 on every level: the restatement's level sizes differ from the halved
    ones (the second aggregation of the denser smoothed operator nearly stalls), and the device gives both."""
    name = "poisson3d(12)"
    n, rp, ci, va = MATRICES[name][0]()
    halved, fixed = restated(name, "host"), restated(name, "host", decay=1.0)
    sizes = lambda levels: [lv["n"] for lv in levels]
    print("poisson3d(12): halved", sizes(halved), "fixed", sizes(fixed))
    assert sizes(halved) != sizes(fixed)
    assert [lv["theta"] for lv in halved[:3]] == [np.float32(0.08), np.float32(0.04), np.float32(0.02)]
    h = Smoothed(gpu, n, rp, ci, va, smoothing=gpu.AMGSmoothing(strength_decay=1.0))
    try:
        assert h.res.error_code == 0
        assert_levels_equal(h.levels(), fixed, "strength_decay = 1")
    finally:
        h.close()
    d = Smoothed(gpu, n, rp, ci, va, smoothing=gpu.AMGSmoothing(strength_decay=1.0), builder="device")
    try:
        assert d.res.error_code == 0
        assert_levels_equal(d.levels(), restated(name, "device", decay=1.0), "strength_decay = 1, device")
    finally:
        d.close()


def test_a_plain_hierarchy_has_the_unit_transfers(gpu):
    n, rp, ci, va = spd.poisson2d(16)
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    res, H = gpu.amg_setup(A)
    try:
        assert res.error_code == 0 and gpu.amg_is_smoothed(H) == 0
        _, _, _, _, agg = gpu.amg_level_arrays(H, 0)
        count = gpu.amg_level(H, 0)[3]
        status, p_view, pt_view = gpu.amg_level_transfer(H, 0)
        assert status == 0
        assert_csr_equal(view_arrays(gpu, p_view), ac.prolongation(n, agg), "the unit P")
        assert_csr_equal(view_arrays(gpu, pt_view), ac.restriction(n, agg, count), "its transpose")
    finally:
        gpu.amg_destroy(H)
        gpu.csr_destroy(A)


# ------------------------------------------------------------------------------------------ the transfers, exact
def exact_cases():
    """name, matrix, maps: level 0 of each is a case the prover admits (tests/test_amg_smoothed_host.py)"""
    yield "tridiagonal(1040), blocks of 260", ac.tridiagonal(1040), [sc.block_map(1040, 260)]
    yield "arrow(300), singletons", sc.arrow(300), [np.arange(300, dtype=np.int32)]
    yield "tridiagonal(64), pairs", ac.tridiagonal(64), ac.pair_maps(64, 32)


class Vectors:
    def __init__(self, gpu, n, count):
        self.gpu, self.n, self.count = gpu, n, count
        self.d_f, self.d_x, self.d_e, self.d_fc = (gpu.CudaBuffer(m) for m in (n, n, count, count))

    def run(self, H, f, x, e):
        gpu = self.gpu
        self.d_f.copyFromHost(f, self.n)
        self.d_x.copyFromHost(x, self.n)
        self.d_e.copyFromHost(e, self.count)
        self.d_fc.copyFromHost(np.full(self.count, np.nan, np.float32), self.count)
        assert gpu.amg_restrict(H, 0, self.d_f, self.d_x, self.d_fc) == 0
        fc = self.d_fc.copyToHost(self.count)
        np.testing.assert_array_equal(bits(self.d_x.copyToHost(self.n)), bits(x))       # the inputs are only read
        np.testing.assert_array_equal(bits(self.d_f.copyToHost(self.n)), bits(f))
        assert gpu.amg_prolong(H, 0, self.d_e, self.d_x) == 0
        return fc, self.d_x.copyToHost(self.n)

    def close(self):
        for b in (self.d_f, self.d_x, self.d_e, self.d_fc):
            b.release()


@pytest.mark.parametrize("case", list(exact_cases()), ids=lambda c: c[0])
def test_exact_transfers_at_every_lane_count(gpu, monkeypatch, case):
    """omega_p = 1/2 and integer f, x, e in [-8, 8]: every term of every sum is a multiple of one power of two, the
    prover bounds the sums, and the device must give integer / Fraction arithmetic bit for bit at 1 .. 64 lanes."""
    name, (n, rp, ci, va), maps = case
    h = Smoothed(gpu, n, rp, ci, va, smoothing=gpu.AMGSmoothing(prolongator_weight=0.5), maps=maps)
    v = None
    try:
        assert h.res.error_code == 0 and h.res.levels == 2
        level = h.levels()[0]
        v = Vectors(gpu, n, level["count"])
        f, x, e = sc.exact_vectors(level)
        want_fc, want_x, width = sc.prove_transfers(level, f, x, e)
        print(f"{name}: " + (f"{width} bits" if want_fc is not None else f"not admitted ({width})"),
              "longest rows of P, PT:", int(np.diff(level["P"][0]).max()), int(np.diff(level["PT"][0]).max()))
        assert want_fc is not None, (name, width)
        for lanes in LANES + (None,):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG")                   # the library's own lane counts
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"amg_lanes={lanes}")
            fc, out = v.run(h.H, f, x, e)
            np.testing.assert_array_equal(bits(fc), bits(want_fc), err_msg=f"{name}: amg_restrict at lanes {lanes}")
            np.testing.assert_array_equal(bits(out), bits(want_x), err_msg=f"{name}: amg_prolong at lanes {lanes}")
    finally:
        if v:
            v.close()
        h.close()


def test_transfers_on_a_plain_hierarchy_follow_the_plain_rule(gpu, monkeypatch):
    """tridiag(-1, 2, -1) with pairs: the restriction adds the two members' residuals, the prolongation gathers"""
    n, rp, ci, va = ac.tridiagonal(64)
    A = gpu.csr_from_arrays(n, n, rp, ci, va)
    assert gpu.csr_to_gpu(A) == 0
    res, H = gpu.amg_setup(A, None, ac.pair_maps(64, 32))
    v = Vectors(gpu, n, 32)
    try:
        assert res.error_code == 0 and res.levels == 2
        rng = np.random.default_rng(9)
        f, x, e = (rng.integers(-8, 9, m).astype(np.float32) for m in (n, n, 32))
        dense = ac.dense_of(dict(n=n, rp=rp, ci=ci, va=va)).astype(np.int64)
        residual = f.astype(np.int64) - dense @ x.astype(np.int64)
        want_fc = (residual[0::2] + residual[1::2]).astype(np.float32)
        want_x = (x.astype(np.int64) + e.astype(np.int64)[np.arange(n) // 2]).astype(np.float32)
        for lanes in LANES + (None,):
            if lanes is None:
                monkeypatch.delenv("SPMV_DEBUG")
            else:
                monkeypatch.setenv("SPMV_DEBUG", f"amg_lanes={lanes}")
            fc, out = v.run(H, f, x, e)
            np.testing.assert_array_equal(bits(fc), bits(want_fc), err_msg=f"lanes {lanes}")
            np.testing.assert_array_equal(bits(out), bits(want_x), err_msg=f"lanes {lanes}")
    finally:
        v.close()
        gpu.amg_destroy(H)
        gpu.csr_destroy(A)


def test_transfer_rejections_write_nothing(gpu):
    E = gpu.SpMVError
    n, rp, ci, va = ac.tridiagonal(64)
    h = Smoothed(gpu, n, rp, ci, va, maps=ac.pair_maps(64, 32))
    v = Vectors(gpu, n, 32)
    try:
        marks = np.arange(n, dtype=np.float32) + 0.5
        for b, m in ((v.d_f, n), (v.d_x, n), (v.d_e, 32), (v.d_fc, 32)):
            b.copyFromHost(marks[:m], m)
        for level in (-1, 1, 2):
            assert gpu.amg_restrict(h.H, level, v.d_f, v.d_x, v.d_fc) == E.INVALID_DIMENSION
            assert gpu.amg_prolong(h.H, level, v.d_e, v.d_x) == E.INVALID_DIMENSION
        assert gpu.amg_restrict(h.H, 0, None, v.d_x, v.d_fc) == E.INVALID_ARGUMENT
        assert gpu.amg_restrict(h.H, 0, v.d_f, None, v.d_fc) == E.INVALID_ARGUMENT
        assert gpu.amg_restrict(h.H, 0, v.d_f, v.d_x, None) == E.INVALID_ARGUMENT
        assert gpu.amg_prolong(h.H, 0, None, v.d_x) == E.INVALID_ARGUMENT
        assert gpu.amg_prolong(h.H, 0, v.d_e, None) == E.INVALID_ARGUMENT
        # the coarse vector inside either input, and e inside x
        assert gpu.amg_restrict(h.H, 0, v.d_f, v.d_x, v.d_f.get() + 4 * 40) == E.INVALID_ARGUMENT
        assert gpu.amg_restrict(h.H, 0, v.d_f, v.d_x, v.d_x.get() + 4 * 16) == E.INVALID_ARGUMENT
        assert gpu.amg_prolong(h.H, 0, v.d_x.get() + 4 * 8, v.d_x) == E.INVALID_ARGUMENT
        for b, m in ((v.d_f, n), (v.d_x, n), (v.d_e, 32), (v.d_fc, 32)):
            np.testing.assert_array_equal(bits(b.copyToHost(m)), bits(marks[:m]))
    finally:
        v.close()
        h.close()


# ------------------------------------------------------------------------------------------ the cycle, by bound
@pytest.mark.parametrize("name", list(MATRICES))
def test_cycle_within_the_distance_of_the_two_restatements(gpu, name):
    make, coarse_rows = MATRICES[name]
    n, rp, ci, va = make()
    h = Smoothed(gpu, n, rp, ci, va, gpu.AMGConfig(coarse_rows=coarse_rows))
    try:
        assert h.res.error_code == 0 and h.res.levels >= 3
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


def test_cycle_with_other_sweep_counts_and_the_device_builder(gpu):
    """no post-sweeps (the prolongation writes the output vector itself), two sweeps each side, and a device-built
    hierarchy"""
    n, rp, ci, va = spd.poisson2d(32)
    for keywords, builder in (({"pre_sweeps": 2, "post_sweeps": 0}, "host"), ({"pre_sweeps": 2, "post_sweeps": 2}, "host"),
                              ({}, "device")):
        h = Smoothed(gpu, n, rp, ci, va, gpu.AMGConfig(**keywords), builder=builder)
        try:
            assert h.res.error_code == 0 and h.res.levels >= 3
            r = np.random.default_rng(13).uniform(-1, 1, n).astype(np.float32)
            z32, z64 = h.reference(r, np.float32), h.reference(r, np.float64)
            z = h.apply(r)
            error = float(np.max(np.abs(z.astype(np.float64) - z64)))
            print(keywords, builder, f"error {error:.3g}, bound {ac.tolerance(z32, z64):.3g}")
            assert np.isfinite(z).all() and error <= ac.tolerance(z32, z64), (keywords, builder)
            np.testing.assert_array_equal(bits(h.apply(r)), bits(z))
        finally:
            h.close()


def test_vectors_that_are_views_at_odd_offsets(gpu):
    n, rp, ci, va = spd.poisson2d(32)
    h = Smoothed(gpu, n, rp, ci, va)
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
        d_in.release()
        d_out.release()
    finally:
        h.close()


# ------------------------------------------------------------------------------------------ amg_update
@pytest.mark.parametrize("builder", ["host", "device"])
def test_update_equals_a_fresh_setup_and_a_wrong_pattern_leaves_the_hierarchy_usable(gpu, builder):
    n, rp, ci, va = spd.poisson2d(32)
    h = Smoothed(gpu, n, rp, ci, va, builder=builder)
    try:
        assert h.res.error_code == 0
        before = h.levels()
        maps = [lv["agg"] for lv in before[:-1]]
        r = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
        # 1.5 A + 0.25 I through another handle: amg_setup_smoothed on it with the same maps, bit for bit
        shifted = (np.float32(1.5) * va + np.where(ci == ac.rows_of(n, rp), np.float32(0.25), np.float32(0))).astype(np.float32)
        fresh = Smoothed(gpu, n, rp, ci, shifted, maps=maps)
        assert fresh.res.error_code == 0
        res = gpu.amg_update(h.H, fresh.A)
        assert res.error_code == 0 and res.levels == len(before) and res.coarse_solver == 0
        assert res.operator_complexity == pytest.approx(fresh.res.operator_complexity)
        updated = h.levels()
        assert_levels_equal(updated, fresh.levels(), f"update against setup, {builder}")
        assert any(not np.array_equal(bits(u["va"]), bits(b["va"])) for u, b in zip(updated[1:], before[1:]))
        np.testing.assert_array_equal(bits(h.apply(r)), bits(fresh.apply(r)))
        # the same number of entries in another pattern: row 0's entry (0, 32) moved to (0, 1000)
        moved = ci.copy()
        where = np.flatnonzero((ac.rows_of(n, rp) == 0) & (ci == 32))
        assert where.size == 1
        moved[where] = 1000
        B = gpu.csr_from_arrays(n, n, rp, moved, va)
        assert gpu.csr_to_gpu(B) == 0
        assert gpu.amg_update(h.H, B).error_code == gpu.SpMVError.INVALID_FORMAT
        gpu.csr_destroy(B)
        # usable again after a good update
        assert gpu.amg_update(h.H, fresh.A).error_code == 0
        assert_levels_equal(h.levels(), fresh.levels(), f"after the rejected update, {builder}")
        np.testing.assert_array_equal(bits(h.apply(r)), bits(fresh.apply(r)))
        fresh.close()
    finally:
        h.close()
