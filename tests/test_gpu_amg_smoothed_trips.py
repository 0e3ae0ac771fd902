"""The smoothed-aggregation AMG (include/spmv/amg.h) past its grid caps, every comparison at zero
tolerance: bits of values, ints of structure.

The family is precond_trip_cases' section 6: tridiag(-1, 2, -1) of even n with pair aggregates, two levels, the
coarsest Jacobi-solved, omega = 1/2 and omega_p = 1, on which every quantity of the weighted cycle is dyadic.
tests/test_amg_smoothed_host.py settles on the CPU that every case is admitted by
precond_trip_cases.prove_smoothed_vcycle_fast and which caps it passes; nothing here is measured first and asserted
afterwards.  R_L = 524 288 / L rows a trip of a row kernel at L lanes, V = 262 144 elements a trip of an element-wise
kernel (csrc/device_common.h).  A and P have n rows, PT and level 1 have n / 2, so each sweep meets its cap at another n.

kernel                                   case that gives it a second trip                      rows in that trip
amg_residual_kernel<64>, amg_prolong_<64>  "L64", n = 16 394: the third trip                     10
amg_restrict_weighted_kernel<64>,          the same: 8197 aggregates and rows of level 1         5
amg_sweep_kernel<64> on level 1
the same four at 8 lanes                   "L8", n = 131 138                                     66; 33
amg_restrict_weighted_kernel<64>           "below", "at", "above": 8191, 8192, 8193 aggregates   none, none (2048 full
                                           while A and P (n = 2 x that) are past R_64            workgroups), 1
amg_scale_kernel                           "vec", n = 2 (V + 257), the library's lanes           V + 514 (fine), 257
amg_residual_kernel<1>, amg_prolong_<1>    the same: one lane for A, P and PT, R_1 = 524 288     514
amg_smoothing_scale_kernel                 amg_setup_smoothed on "vec"; _device on V + 257 rows  V + 514; 257
spgemm_csr_numeric, csr_add_numeric,       amg_update of the "vec" hierarchy
csr_scale_gpu, csr_transpose_gpu

The residual the cycle stores is not readable through the interface; every row of it enters one or two sums of PT r
with the weight 1/2, so a wrong or missing row changes the restricted vector, which is compared."""
import importlib

import numpy as np
import pytest

import amg_cases as ac
import amg_smoothed_cases as sc
import exact_data as ed
import precond_trip_cases as pt

pytestmark = pytest.mark.gpu

smoothed_tests = importlib.import_module("test_gpu_amg_smoothed")
trip_tests = importlib.import_module("test_gpu_precond_trips")
Smoothed, assert_levels_equal = smoothed_tests.Smoothed, smoothed_tests.assert_levels_equal
forced, assert_bits, apply_through_views = trip_tests.forced, trip_tests.assert_bits, trip_tests.apply_through_views


class Case:
    """A case of pt.SMOOTHED_CASES: the matrix, the maps, the right-hand side and the host-twin levels, built once"""

    def __init__(self, spmv, name):
        self.name = name
        self.n, self.lanes, self.sweep_counts = pt.SMOOTHED_CASES[name]
        self.matrix = pt.tridiagonal(self.n)
        self.maps = ac.pair_maps(self.n, self.n // 2)
        self.r = ac.exact_rhs(self.n)
        self.levels = pt.smoothed_hierarchy(spmv, self.n)
        self.proved = {}

    def debug(self):
        return None if self.lanes is None else f"amg_lanes={self.lanes}"

    def want(self, pre, coarse, post):
        if (pre, coarse, post) not in self.proved:
            z, width = pt.prove_smoothed_vcycle_fast(self.levels, self.r, pt.AMG_OMEGA, pre, post, coarse)
            assert z is not None, (self.name, pre, coarse, post, width)
            z.setflags(write=False)
            self.proved[pre, coarse, post] = z
        return self.proved[pre, coarse, post]

    def hierarchy(self, gpu, pre=1, coarse=1, post=1, va=None):
        cfg = gpu.AMGConfig(jacobi_weight=pt.AMG_OMEGA, pre_sweeps=pre, post_sweeps=post, coarse_sweeps=coarse)
        n, rp, ci, own = self.matrix
        h = Smoothed(gpu, n, rp, ci, own if va is None else va, cfg,
                     gpu.AMGSmoothing(prolongator_weight=pt.SMOOTHED_WEIGHT), self.maps)
        assert (h.res.error_code, h.res.levels, h.res.coarse_solver) == (0, 2, 1), (self.name, h.res.error_code)
        return h


@pytest.fixture(scope="module")
def cases(gpu):
    built = {}

    def get(name):
        if name not in built:
            built[name] = Case(gpu, name)
        return built[name]
    return get


def picked_lanes(gpu, h):
    """pick_lanes_per_row (exact_data.lanes_for restates it) of A, P, PT on level 0 and of A on level 1"""
    status, p_view, pt_view = gpu.amg_level_transfer(h.H, 0)
    assert status == 0
    fine, coarse = gpu.amg_level(h.H, 0)[1], gpu.amg_level(h.H, 1)[1]
    return [ed.lanes_for(m.nnz, m.num_rows) for m in (fine, p_view, pt_view, coarse)]


# ------------------------------------------------------------------------------------------ the transfers
@pytest.mark.parametrize("name", list(pt.SMOOTHED_CASES))
def test_transfers_past_the_caps(gpu, cases, name):
    """amg_restrict and amg_prolong on level 0 (Cycle::down and Cycle::up, the cycle's own launches) with integer f, x
    and e: PT (f - A x) and x + P e are the prover's bits; amg_prolong runs in place; the inputs stay as uploaded."""
    case = cases(name)
    level = case.levels[0]
    f, x, e = sc.exact_vectors(level)
    _, want_fc, want_x, width = pt.prove_smoothed_transfers_fast(level, f, x, e)
    assert want_fc is not None, (name, width)
    h = case.hierarchy(gpu)
    v = smoothed_tests.Vectors(gpu, case.n, level["count"])
    try:
        with forced(case.debug()):
            fc, out = v.run(h.H, f, x, e)                 # asserts f and x intact after the restriction
            assert_bits(fc, want_fc, (name, "amg_restrict"))
            assert_bits(out, want_x, (name, "amg_prolong"))
            assert_bits(v.d_f.copyToHost(case.n), f, (name, "f after both"))
            assert_bits(v.d_e.copyToHost(level["count"]), e, (name, "e after amg_prolong"))
            fc, out = v.run(h.H, f, x, e)
            assert_bits(fc, want_fc, (name, "amg_restrict again"))
            assert_bits(out, want_x, (name, "amg_prolong again"))
    finally:
        v.close()
        h.close()


# ------------------------------------------------------------------------------------------ the whole cycle
@pytest.mark.parametrize("name", list(pt.SMOOTHED_CASES))
def test_smoothed_vcycle_every_kernel_past_its_cap(gpu, cases, name):
    """amg_apply is the proved vector for every sweep shape of the case, twice, and through views 3 floats into NaN-
    and marker-padded buffers (guards and input asserted intact)."""
    case = cases(name)
    for pre, coarse, post in case.sweep_counts:
        want = case.want(pre, coarse, post)
        h = case.hierarchy(gpu, pre, coarse, post)
        try:
            if case.lanes is None:
                print(f"{name}: lanes the library picks for A, P, PT of level 0 and A of level 1:", picked_lanes(gpu, h))
            with forced(case.debug()):
                what = (name, pre, coarse, post)
                assert_bits(h.apply(case.r), want, what)
                assert_bits(h.apply(case.r), want, what + ("again",))
                assert_bits(apply_through_views(gpu, h, case.r), want, what + ("views",))
        finally:
            h.close()


# ------------------------------------------------------------------------------------------ the builders at size
def test_smoothed_setup_past_the_vector_cap(gpu, cases):
    """amg_setup_smoothed with the pair maps on 2 (V + 257) rows: both levels, P and PT are the chain of host twins"""
    case = cases("vec")
    h = case.hierarchy(gpu)
    try:
        assert gpu.amg_is_smoothed(h.H) == 1
        assert_levels_equal(h.levels(), case.levels, "amg_setup_smoothed on the vec case")
    finally:
        h.close()


def test_smoothed_device_setup_past_the_vector_cap(gpu):
    """amg_setup_smoothed_device on tridiag(-1, 2, -1) of V + 257 rows, max_levels = 2, the default omega_p: equal to
    amg_setup_smoothed handed the definition's map (amg_aggregate_mis2_cpu_csr) and to the chain of host twins on that
    map, bit for bit; one cycle of each hierarchy gives the same bits."""
    n, rp, ci, va = pt.tridiagonal(pt.VEC_ROWS)
    cfg = gpu.AMGConfig(max_levels=2)
    host_A = gpu.csr_from_arrays(n, n, rp, ci, va)
    status, agg, count, _ = gpu.amg_aggregate_mis2_cpu_csr(host_A, cfg.strength, smoothed_tests.SEED)
    gpu.csr_destroy(host_A)
    assert status == 0 and ac.DENSE_ROWS < count < n
    dev = Smoothed(gpu, n, rp, ci, va, cfg, builder="device")
    host = Smoothed(gpu, n, rp, ci, va, cfg, maps=[agg])
    try:
        assert dev.res.error_code == 0 and dev.H is not None and (dev.res.bad_row, dev.res.bad_level) == (-1, -1)
        assert host.res.error_code == 0
        assert (dev.res.levels, dev.res.coarse_solver) == (host.res.levels, host.res.coarse_solver) == (2, 1)
        got, want = dev.levels(), host.levels()
        assert got[1]["n"] == count
        assert_levels_equal(got, want, "the device-built smoothed hierarchy")
        assert_levels_equal(got, sc.hierarchy(gpu, n, rp, ci, va, maps=[agg], max_levels=2), "the chain of host twins")
        r = ac.exact_rhs(n)
        assert_bits(dev.apply(r), host.apply(r), "one V-cycle of each hierarchy")
    finally:
        dev.close()
        host.close()


# ------------------------------------------------------------------------------------------ the refill at size
def test_smoothed_update_past_the_vector_cap(gpu, cases):
    """amg_update of the vec hierarchy with 1.5 A + 0.25 I through a second handle equals a fresh amg_setup_smoothed on
    that matrix with the same maps (levels, P, PT, one amg_apply); updated back with A, the proved cycle comes out
    again and the levels are the host twins': nothing stale survives two refills."""
    case = cases("vec")
    pre, coarse, post = case.sweep_counts[0]
    want = case.want(pre, coarse, post)
    n, rp, ci, va = case.matrix
    shifted = (np.float32(1.5) * va + np.where(ci == ac.rows_of(n, rp), np.float32(0.25), np.float32(0))).astype(np.float32)
    h = case.hierarchy(gpu, pre, coarse, post)
    fresh = case.hierarchy(gpu, pre, coarse, post, va=shifted)
    try:
        assert_bits(h.apply(case.r), want, "before the update")
        res = gpu.amg_update(h.H, fresh.A)
        assert (res.error_code, res.levels, res.coarse_solver) == (0, 2, 1)
        updated, expected = h.levels(), fresh.levels()
        assert_levels_equal(updated, expected, "amg_update against a fresh setup")
        assert not np.array_equal(updated[1]["va"], case.levels[1]["va"])
        assert_bits(h.apply(case.r), fresh.apply(case.r), "one V-cycle after the update")
        res = gpu.amg_update(h.H, h.A)
        assert (res.error_code, res.levels, res.coarse_solver) == (0, 2, 1)
        assert_levels_equal(h.levels(), case.levels, "after the update back")
        assert_bits(h.apply(case.r), want, "the proved cycle after two refills")
    finally:
        h.close()
        fresh.close()
