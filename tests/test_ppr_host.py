"""pagerank_personalized / pagerank_personalized_seeds (include/spmv/pagerank.h) on the host side (no GPU): the
exported names, the struct layout and the eight argument checks that come before any device work, in their documented
order, through the C ABI and the Python wrapper.  Pairs of faults show which check wins.  V, R and `results` are host
memory standing in for device arrays, as in tests/test_cg_multi_host.py: a rejected call must leave R untouched and
write nothing to `results` but error_code."""
import ctypes

import numpy as np

from test_cg_host import _device_header, _host_matrix

K_MAX = 32
POISON = np.float32(-7.25)


class Arrays:
    """Host stand-ins: V and R of `rows` x `ld` floats, far apart in one allocation, and `count` poisoned results."""

    def __init__(self, spmv, rows=8, ld=K_MAX + 1, count=K_MAX + 1):
        self.store = np.full(4 * rows * ld, POISON, np.float32)
        self.V = self.store.ctypes.data
        self.R = self.V + 4 * 2 * rows * ld
        self.results = (spmv.PersonalizedResult * count)()
        for r in self.results:
            r.error_code, r.iterations, r.final_residual, r.converged, r.elapsed_ms = 12345, 77, 0.5, 9, 2.5

    def assert_untouched(self, written, code):
        assert np.all(self.store == POISON)
        for j, r in enumerate(self.results):
            assert r.error_code == (code if j < written else 12345), (j, r.error_code)
            assert (r.iterations, r.final_residual, r.converged, r.elapsed_ms) == (77, 0.5, 9, 2.5)


def _c_call(spmv, A, V, ldv, R, ldr, k, cfg, results):
    return spmv.lib().spmv_c_pagerank_personalized(A, ctypes.c_void_p(V), ldv, ctypes.c_void_p(R), ldr, k,
                                                   ctypes.byref(cfg) if cfg is not None else None, results)


def _c_seeds(spmv, A, ptrs, nodes, k, R, ldr, cfg, results):
    ptrs = None if ptrs is None else np.asarray(ptrs, np.int32)
    nodes = None if nodes is None else np.asarray(nodes, np.int32)
    return spmv.lib().spmv_c_pagerank_personalized_seeds(
        A, None if ptrs is None else ptrs.ctypes.data_as(ctypes.c_void_p),
        None if nodes is None else nodes.ctypes.data_as(ctypes.c_void_p), k, ctypes.c_void_p(R), ldr,
        ctypes.byref(cfg) if cfg is not None else None, results)


def test_names_exist_in_the_c_abi_and_the_python_mirror(spmv):
    for name in ("spmv_c_pagerank_personalized", "spmv_c_pagerank_personalized_seeds"):
        assert name in spmv.EXPORTED_SYMBOLS
        assert hasattr(spmv.lib(), name)
    assert callable(spmv.pagerank_personalized) and callable(spmv.pagerank_personalized_seeds)


def test_result_layout(spmv):
    assert ctypes.sizeof(spmv.PersonalizedResult) == 20
    assert [f for f, _ in spmv.PersonalizedResult._fields_] == ["error_code", "iterations", "final_residual",
                                                                "converged", "elapsed_ms"]
    assert spmv.PersonalizedResult.elapsed_ms.offset == 16


def test_checks_in_the_stated_order_through_the_c_abi(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.PageRankConfig(damping_factor=1.5)
    A = _host_matrix(spmv)                        # square, host only: INVALID_FORMAT at check 6
    R = spmv.csr_create(5, 4, 0)                  # not square
    Z = spmv.csr_create(0, 0, 0)                  # empty
    D = _device_header(spmv)                      # passes 1..6
    try:
        def call(M, V, ldv, Rp, ldr, k, cfg, results, written):
            rc = _c_call(spmv, M, V, ldv, Rp, ldr, k, cfg, results)
            a.assert_untouched(written if results is not None else 0, rc)
            for r in a.results:
                r.error_code = 12345
            return rc

        # 1. nulls, before k (0 and 33 are bad), the leading dimensions, the shape, everything
        for k in (0, 4, K_MAX + 1):
            written = k if 1 <= k <= K_MAX else 0
            assert call(None, a.V, 1, a.R, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, None, 1, a.R, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, a.V, 1, None, 1, k, bad_cfg, a.results, written) == E.INVALID_ARGUMENT
            assert call(R, a.V, 1, a.R, 1, k, bad_cfg, None, 0) == E.INVALID_ARGUMENT
        # 2. k, before the leading dimensions and the shape (INVALID_DIMENSION would win otherwise)
        for k in (0, -1, K_MAX + 1, 1 << 20):
            assert call(R, a.V, 40, a.R, 40, k, bad_cfg, a.results, 0) == E.INVALID_ARGUMENT
        # 3. leading dimensions, before the shape
        assert call(R, a.V, 3, a.R, 4, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
        assert call(R, a.V, 4, a.R, 3, 4, bad_cfg, a.results, 4) == E.INVALID_ARGUMENT
        assert call(Z, a.V, 0, a.R, 4, 1, bad_cfg, a.results, 1) == E.INVALID_ARGUMENT      # before the empty graph
        # 4. not square, before the empty and format checks
        assert call(R, a.V, 4, a.R, 4, 4, bad_cfg, a.results, 4) == E.INVALID_DIMENSION
        R0 = spmv.csr_create(0, 3, 0)
        assert call(R0, a.V, 4, a.R, 4, 4, bad_cfg, a.results, 4) == E.INVALID_DIMENSION
        spmv.csr_destroy(R0)
        # 6. missing device arrays, before the config and the overlap
        assert call(A, a.V, 4, a.R, 4, 4, bad_cfg, a.results, 4) == E.INVALID_FORMAT
        assert call(A, a.V, 4, a.V, 4, 4, None, a.results, 4) == E.INVALID_FORMAT
        # 7. config values, before the overlap
        for cfg in (spmv.PageRankConfig(damping_factor=0.0), spmv.PageRankConfig(damping_factor=1.0),
                    spmv.PageRankConfig(damping_factor=-0.5), spmv.PageRankConfig(damping_factor=float("nan")),
                    spmv.PageRankConfig(tolerance=-1e-3), spmv.PageRankConfig(tolerance=float("nan")),
                    spmv.PageRankConfig(tolerance=float("inf")), spmv.PageRankConfig(max_iterations=-1)):
            assert call(D, a.V, 4, a.V, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
            assert call(D, a.V, 4, a.R, 4, 4, cfg, a.results, 4) == E.INVALID_ARGUMENT
        # 8. overlap of [V, V + (n - 1) ldv + k) and [R, R + (n - 1) ldr + k): n = 8, k = 3, ldv = 5 -> 38 floats of V,
        #    ldr = 4 -> 31 floats of R; a null config takes the defaults
        for cfg in (None, spmv.PageRankConfig(), spmv.PageRankConfig(0.5, 0.0, 0)):
            for r in (a.V, a.V + 4, a.V + 4 * 37, a.V - 4 * 30):
                assert call(D, a.V, 5, r, 4, 3, cfg, a.results, 3) == E.INVALID_ARGUMENT
    finally:
        for M in (A, R, Z, D):
            spmv.csr_destroy(M)


def test_the_same_order_through_python(spmv):
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.PageRankConfig(tolerance=-1.0)
    A, R, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), _device_header(spmv)
    try:
        def codes(*args, **kw):
            out = spmv.pagerank_personalized(*args, **kw)
            assert np.all(a.store == POISON)
            assert isinstance(out, list) and len(out) >= 1
            assert len({r.error_code for r in out}) == 1
            assert all((r.iterations, r.converged, r.final_residual, r.elapsed_ms) == (0, 0, 0.0, 0.0) for r in out)
            return out[0].error_code, len(out)

        assert codes(None, a.V, a.R, 0, config=bad_cfg) == (E.INVALID_ARGUMENT, 1)              # null before k
        assert codes(R, None, a.R, 4, ldv=1, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.V, None, 4, ldr=1, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.V, a.R, 0, config=bad_cfg) == (E.INVALID_ARGUMENT, 1)                 # k before the shape
        assert codes(R, a.V, a.R, K_MAX + 1, config=bad_cfg) == (E.INVALID_ARGUMENT, K_MAX + 1)
        assert codes(R, a.V, a.R, 4, ldv=3, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)          # ld before the shape
        assert codes(R, a.V, a.R, 4, ldr=3, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(R, a.V, a.R, 4, config=bad_cfg) == (E.INVALID_DIMENSION, 4)                # shape before format
        assert codes(A, a.V, a.V, 4, config=bad_cfg) == (E.INVALID_FORMAT, 4)                   # format before config
        assert codes(D, a.V, a.V, 4, config=bad_cfg) == (E.INVALID_ARGUMENT, 4)
        assert codes(D, a.V, a.V + 4 * 37, 3, ldv=5, ldr=4) == (E.INVALID_ARGUMENT, 3)          # overlap, good config
        assert codes(D, a.V, a.V - 4 * 30, 3, ldv=5, ldr=4, config=spmv.PageRankConfig()) == (E.INVALID_ARGUMENT, 3)
    finally:
        for M in (A, R, D):
            spmv.csr_destroy(M)


def test_empty_graph_gives_k_converged_results(spmv):
    """num_rows == 0 comes after the k / ld / shape checks and before the format, config and overlap checks."""
    E = spmv.SpMVError
    bad_cfg = spmv.PageRankConfig(tolerance=-1.0)
    Z = spmv.csr_create(0, 0, 0)
    try:
        for k in (1, 5, K_MAX):
            a = Arrays(spmv)
            assert _c_call(spmv, Z, a.V, k, a.V, k, k, bad_cfg, a.results) == E.SUCCESS
            assert np.all(a.store == POISON)
            for j, r in enumerate(a.results):
                if j < k:
                    assert (r.error_code, r.iterations, r.converged) == (E.SUCCESS, 0, 1)
                    assert r.final_residual == 0.0 and r.elapsed_ms == 0.0
                else:
                    assert (r.error_code, r.iterations, r.converged) == (12345, 77, 9)
            out = spmv.pagerank_personalized(Z, a.V, a.V, k, config=bad_cfg)
            assert len(out) == k
            assert all((r.error_code, r.iterations, r.converged) == (E.SUCCESS, 0, 1) for r in out)
            a = Arrays(spmv)
            assert _c_seeds(spmv, Z, np.arange(k + 1), np.zeros(k), k, a.R, k, bad_cfg, a.results) == E.SUCCESS
            assert np.all(a.store == POISON) and a.results[k - 1].converged == 1 and a.results[k].converged == 9
    finally:
        spmv.csr_destroy(Z)


def test_seed_sets_are_checked_on_the_host(spmv):
    """The seeds entry point runs the same checks (the sets stand in for V), then the sets: an empty set, a node out of
    range, a node twice in one set.  D's device arrays are fake addresses: every call must return before it touches
    them.  The same node in two different sets is allowed, and only then would device work begin (not tried here)."""
    E = spmv.SpMVError
    a = Arrays(spmv)
    bad_cfg = spmv.PageRankConfig(damping_factor=2.0)
    A, R, D = _host_matrix(spmv), spmv.csr_create(5, 4, 0), _device_header(spmv)       # n = 8
    try:
        def call(M, ptrs, nodes, k, Rp, ldr, cfg, results, written):
            rc = _c_seeds(spmv, M, ptrs, nodes, k, Rp, ldr, cfg, results)
            a.assert_untouched(written if results is not None else 0, rc)
            for r in a.results:
                r.error_code = 12345
            return rc

        good = ([0, 1, 3], [2, 4, 5])
        assert call(None, *good, 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT
        assert call(R, None, good[1], 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT
        assert call(R, good[0], None, 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT
        assert call(R, *good, 2, None, 2, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT
        assert call(R, *good, 2, a.R, 2, bad_cfg, None, 0) == E.INVALID_ARGUMENT
        assert call(R, *good, 0, a.R, 2, bad_cfg, a.results, 0) == E.INVALID_ARGUMENT
        assert call(R, *good, K_MAX + 1, a.R, 40, bad_cfg, a.results, 0) == E.INVALID_ARGUMENT
        assert call(R, *good, 2, a.R, 1, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT            # ldr before the shape
        assert call(R, *good, 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_DIMENSION
        assert call(A, [0, 0, 1], [9, 9], 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_FORMAT  # format before the sets
        assert call(D, [0, 0, 1], [9, 9], 2, a.R, 2, bad_cfg, a.results, 2) == E.INVALID_ARGUMENT
        for ptrs, nodes in (([0, 0, 2], [1, 2]),              # an empty set
                            ([0, 2, 2], [1, 2]),
                            ([0, 1, 3], [2, 4, 8]),           # n = 8: node 8 is out of range
                            ([0, 1, 3], [-1, 4, 5]),
                            ([0, 1, 3], [2, 4, 4]),           # twice in one set
                            ([0, 3, 4], [6, 1, 6, 2])):
            assert call(D, ptrs, nodes, 2, a.R, 2, None, a.results, 2) == E.INVALID_ARGUMENT, (ptrs, nodes)
        out = spmv.pagerank_personalized_seeds(D, [[2], [4, 4]], a.R)
        assert [r.error_code for r in out] == [E.INVALID_ARGUMENT] * 2 and np.all(a.store == POISON)
        out = spmv.pagerank_personalized_seeds(D, [[2], []], a.R)
        assert [r.error_code for r in out] == [E.INVALID_ARGUMENT] * 2
        out = spmv.pagerank_personalized_seeds(D, [], a.R)
        assert len(out) == 1 and out[0].error_code == E.INVALID_ARGUMENT
    finally:
        for M in (A, R, D):
            spmv.csr_destroy(M)
