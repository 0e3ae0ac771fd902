"""minres_solve / minres_solve_ic (include/spmv/minres.h) on the host side (no GPU): the exported names, the struct
layouts and defaults, the argument checks that come before any device work, in their documented order, through the C
ABI and the Python wrapper, the numpy restatement of the header's rules (tests/minres_cases.py) against fp64, and the
proof in integer / Fraction arithmetic that the exact families of tests/test_gpu_minres_exact.py are exact."""
import ctypes

import numpy as np
import pytest

import exact_data as ed
import minres_cases as mc


def _host_matrix(spmv, rows=8, cols=8):
    A = spmv.csr_create(0, 0, 0)
    dense = np.zeros((rows, cols), np.float32)
    for i in range(rows):
        dense[i, i % cols] = -4.0
        dense[i, (i + 1) % cols] = 1.0
    assert spmv.csr_from_dense(A, dense, rows, cols) == 0
    return A


# fake, never-dereferenced device addresses: every call below must return before it touches them
B, X = 0x100000, 0x200000
FAKE_RP, FAKE_CI, FAKE_VA = 0x300000, 0x400000, 0x500000


def _device_header(spmv, n=8, nnz=16):
    return spmv.csr_wrap_device(n, n, nnz, FAKE_RP, FAKE_CI, FAKE_VA)


def test_names_exist_in_the_c_abi_the_library_and_python(spmv):
    for name in ("spmv_c_minres_solve", "spmv_c_minres_solve_ic"):
        assert name in spmv.EXPORTED_SYMBOLS
        assert hasattr(spmv.lib(), name)
    assert callable(spmv.minres_solve) and callable(spmv.minres_solve_ic)
    assert (spmv.MINRES_NO_BREAKDOWN, spmv.MINRES_PRECONDITIONER, spmv.MINRES_NOT_FINITE, spmv.MINRES_SINGULAR) == \
        (0, 1, 2, 3)
    R = spmv.MinresResult
    assert (R.NONE, R.PRECONDITIONER, R.NOT_FINITE, R.SINGULAR) == (0, 1, 2, 3)
    assert (spmv.MinresConfig.NONE, spmv.MinresConfig.JACOBI) == (spmv.CGConfig.NONE, spmv.CGConfig.JACOBI)
    assert (mc.NO_BREAKDOWN, mc.PRECONDITIONER, mc.NOT_FINITE, mc.SINGULAR) == \
        (R.NONE, R.PRECONDITIONER, R.NOT_FINITE, R.SINGULAR)
    assert (mc.NONE, mc.JACOBI) == (spmv.MinresConfig.NONE, spmv.MinresConfig.JACOBI)


def test_struct_sizes_offsets_and_defaults(spmv):
    C, R = spmv.MinresConfig, spmv.MinresResult
    assert ctypes.sizeof(C) == 20 and ctypes.sizeof(R) == 28
    assert [f for f, _ in C._fields_] == ["tolerance", "max_iterations", "preconditioner", "engine", "shift"]
    assert [f for f, _ in R._fields_] == ["error_code", "iterations", "relative_residual", "true_relative_residual",
                                          "converged", "breakdown", "elapsed_ms"]
    assert (C.tolerance.offset, C.max_iterations.offset, C.preconditioner.offset, C.engine.offset,
            C.shift.offset) == (0, 4, 8, 12, 16)
    assert (R.error_code.offset, R.iterations.offset, R.relative_residual.offset, R.true_relative_residual.offset,
            R.converged.offset, R.breakdown.offset, R.elapsed_ms.offset) == (0, 4, 8, 12, 16, 20, 24)
    c = C()
    assert (np.float32(c.tolerance), c.max_iterations, c.preconditioner, c.engine, c.shift) == \
        (np.float32(1e-6), 1000, 1, -1, 0.0)
    r = R()
    assert (r.error_code, r.iterations, r.converged, r.breakdown, r.relative_residual,
            r.true_relative_residual) == (0, 0, 0, 0, 0.0, 0.0)


def _c_call(spmv, A, b, x, cfg):
    out = spmv.MinresResult(error_code=12345)
    rc = spmv.lib().spmv_c_minres_solve(A, ctypes.c_void_p(b), ctypes.c_void_p(x),
                                        ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def _c_call_ic(spmv, A, F, b, x, cfg):
    out = spmv.MinresResult(error_code=12345)
    rc = spmv.lib().spmv_c_minres_solve_ic(A, F, ctypes.c_void_p(b), ctypes.c_void_p(x),
                                           ctypes.byref(cfg) if cfg is not None else None, ctypes.byref(out))
    assert rc == out.error_code
    return out


def test_checks_in_the_stated_order_through_the_c_abi_and_python(spmv):
    E = spmv.SpMVError
    Cfg = spmv.MinresConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, b, x, cfg=None: _c_call(spmv, A, b, x, cfg),
                 lambda A, b, x, cfg=None: spmv.minres_solve(A, b, x, cfg)):
        A = _host_matrix(spmv)
        # 1. nulls, before everything else
        assert call(None, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, None, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(A, B, None, bad_cfg).error_code == E.INVALID_ARGUMENT
        # 2. not square, before the empty and format checks
        for rows, cols in ((0, 3), (5, 4)):
            R = spmv.csr_create(rows, cols, 0)
            assert call(R, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
            spmv.csr_destroy(R)
        # 3. empty system: converged after 0 iterations, whatever the config and even with b and x the same
        Z = spmv.csr_create(0, 0, 0)
        res = call(Z, B, B, bad_cfg)
        assert (res.error_code, res.converged, res.iterations, res.breakdown) == (E.SUCCESS, 1, 0, 0)
        spmv.csr_destroy(Z)
        # 4. missing device arrays (host-only matrix), before the config and the overlap check
        assert call(A, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        assert call(A, B, B).error_code == E.INVALID_FORMAT
        for rp, ci, va in ((FAKE_RP, None, FAKE_VA), (FAKE_RP, FAKE_CI, None)):
            D = spmv.csr_wrap_device(8, 8, 16, rp, ci, va)
            assert call(D, B, X).error_code == E.INVALID_FORMAT
            spmv.csr_destroy(D)
        # 5. config values, a shift that is not finite among them, before the overlap check
        D = _device_header(spmv)
        for cfg in (Cfg(tolerance=-1e-3), Cfg(tolerance=float("nan")), Cfg(max_iterations=-1), Cfg(preconditioner=2),
                    Cfg(preconditioner=-1), Cfg(engine=2), Cfg(engine=-2), Cfg(shift=float("nan")),
                    Cfg(shift=float("inf")), Cfg(shift=float("-inf"))):
            assert call(D, B, B, cfg).error_code == E.INVALID_ARGUMENT
            assert call(D, B, X, cfg).error_code == E.INVALID_ARGUMENT
        # 6. overlapping b and x ranges (8 floats = 32 bytes each)
        for x in (B, B + 4, B + 28, B - 28):
            assert call(D, B, x).error_code == E.INVALID_ARGUMENT
            assert call(D, B, x, Cfg(preconditioner=0, engine=0, shift=-2.5)).error_code == E.INVALID_ARGUMENT
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_ic_checks_in_the_stated_order(spmv):
    """minres_solve's checks in their order, then cg_solve_ic's additions for F"""
    E = spmv.SpMVError
    Cfg = spmv.MinresConfig
    bad_cfg = Cfg(tolerance=-1.0)
    for call in (lambda A, F, b, x, cfg=None: _c_call_ic(spmv, A, F, b, x, cfg),
                 lambda A, F, b, x, cfg=None: spmv.minres_solve_ic(A, F, b, x, cfg)):
        A = _host_matrix(spmv)
        D = _device_header(spmv)
        # A's own checks first, whatever F is
        assert call(None, D, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        R = spmv.csr_create(5, 4, 0)
        assert call(R, None, B, X, bad_cfg).error_code == E.INVALID_DIMENSION
        assert call(A, None, B, X, bad_cfg).error_code == E.INVALID_FORMAT
        # the config (the preconditioner field is not read, the shift is) and the overlap, before F is looked at
        assert call(D, None, B, X, bad_cfg).error_code == E.INVALID_ARGUMENT
        assert call(D, R, B, X, Cfg(shift=float("nan"))).error_code == E.INVALID_ARGUMENT
        assert call(D, R, B, B + 4, Cfg(preconditioner=7)).error_code == E.INVALID_ARGUMENT
        # then F: null, not square or another size, no device arrays
        assert call(D, None, B, X, Cfg(preconditioner=7)).error_code == E.INVALID_ARGUMENT
        assert call(D, R, B, X, Cfg(preconditioner=7)).error_code == E.INVALID_DIMENSION
        D9 = _device_header(spmv, n=9)
        assert call(D, D9, B, X).error_code == E.INVALID_DIMENSION
        spmv.csr_destroy(D9)
        assert call(D, A, B, X).error_code == E.INVALID_FORMAT
        spmv.csr_destroy(R)
        spmv.csr_destroy(D)
        spmv.csr_destroy(A)


def test_error_code_is_written_through_out_and_out_may_be_null(spmv):
    A = _host_matrix(spmv)
    out = spmv.MinresResult(error_code=7, iterations=9, breakdown=2, true_relative_residual=3.0)
    assert spmv.lib().spmv_c_minres_solve(A, ctypes.c_void_p(B), None, None, ctypes.byref(out)) == \
        spmv.SpMVError.INVALID_ARGUMENT
    assert (out.error_code, out.iterations, out.breakdown, out.true_relative_residual) == \
        (spmv.SpMVError.INVALID_ARGUMENT, 0, 0, 0.0)
    assert spmv.lib().spmv_c_minres_solve(A, ctypes.c_void_p(B), ctypes.c_void_p(X), None, None) == \
        spmv.SpMVError.INVALID_FORMAT
    spmv.csr_destroy(A)


# ------------------------------------------------------------------------------------------ the restatement
def _preconditioners(name):
    return (mc.NONE,) if name in mc.NO_JACOBI else (mc.NONE, mc.JACOBI)


def minres64(D, dinv, b, tol, max_iter):
    """Paige-Saunders MINRES in fp64 on the dense matrix D with M^-1 = diag(dinv): the numpy reference.  Returns
    (x, iterations, converged)."""
    n = b.size
    x = np.zeros(n)
    r1 = r2 = b.astype(np.float64)
    y = dinv * r2
    beta = np.sqrt(r2 @ y)
    thr = tol * beta
    oldb = dbar = epsln = 0.0
    phibar, cs, sn = beta, -1.0, 0.0
    w = w2 = np.zeros(n)
    for k in range(max_iter):
        v = y / beta
        y = D @ v
        if k > 0:
            y = y - (beta / oldb) * r1
        alpha = v @ y
        y = y - (alpha / beta) * r2
        r1, r2 = r2, y
        y = dinv * r2
        oldb, beta = beta, np.sqrt(r2 @ y)
        oldeps, delta, gbar = epsln, cs * dbar + sn * alpha, sn * dbar - cs * alpha
        epsln, dbar = sn * beta, -cs * beta
        gamma = np.sqrt(gbar * gbar + beta * beta)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2 = w2, w
        w = (v - oldeps * w1 - delta * w2) / gamma
        x = x + phi * w
        if phibar <= thr or beta == 0:
            return x, k + 1, True
    return x, max_iter, False


@pytest.mark.parametrize("name", list(mc.SYSTEMS))
def test_restatement_against_fp64(name):
    """Where the fp64 reference converges to the tolerance within the cap, the restatement does too, and its x agrees
    with the fp64 dense solve to its own true residual: ||x - x*|| <= ||A^-1|| ||r||.  The step counts are printed, not
    compared: Lanczos vectors kept in fp32 lose their orthogonality sooner than fp64 ones, which delays convergence
    (983 steps against 866 on indefinite_500, NONE)."""
    (n, rp, ci, va), shift = mc.SYSTEMS[name]()
    b = mc.rhs(n)
    D = mc.dense_of(n, rp, ci, va, shift)
    x_star = np.linalg.solve(D, b.astype(np.float64))
    inv_norm = 1.0 / np.abs(np.linalg.eigvalsh(D)).min()
    tol, cap = 1e-5, 4000
    for precond in _preconditioners(name):
        dinv = mc.jacobi_dinv(n, rp, ci, va, shift).astype(np.float64) if precond == mc.JACOBI else np.ones(n)
        x64, it64, conv64 = minres64(D, dinv, b, tol, cap)
        x, it, conv, brk, rel = mc.restate(n, rp, ci, va, b, np.zeros(n), tol, cap, precond, shift)
        true = mc.true_residual(rp, ci, va, b, x, shift)
        print(name, precond, "fp64 steps", it64, conv64, "restatement", it, conv, brk, rel, "true", true)
        assert brk == mc.NO_BREAKDOWN
        if not conv64:
            continue
        assert conv and rel <= tol
        err = np.linalg.norm(x.astype(np.float64) - x_star)
        assert err <= inv_norm * true * np.linalg.norm(b.astype(np.float64)) * (1 + 1e-6) + 1e-6 * np.linalg.norm(x_star)


@pytest.mark.parametrize("name", list(mc.SYSTEMS))
def test_restatement_residual_never_increases(name):
    (n, rp, ci, va), shift = mc.SYSTEMS[name]()
    b = mc.rhs(n)
    for precond in _preconditioners(name):
        rels = [mc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, k, precond, shift)[4] for k in range(0, 13)]
        assert rels[0] == 1.0 and all(later <= earlier for earlier, later in zip(rels, rels[1:])), (name, precond, rels)
        assert rels[-1] < rels[0]


def test_restatement_edge_cases():
    (n, rp, ci, va), shift = mc.SYSTEMS["indefinite_500"]()
    b = mc.rhs(n)
    x0 = np.full(n, 0.25, np.float32)
    # max_iterations = 0: the guess with its residual
    x, it, conv, brk, rel = mc.restate(n, rp, ci, va, b, x0, 1e-6, 0, mc.JACOBI)
    assert (it, conv, brk) == (0, False, 0) and np.array_equal(x, x0) and rel > 0
    # ||b|| = 0
    x, it, conv, brk, rel = mc.restate(n, rp, ci, va, np.zeros(n, np.float32), x0, 1e-6, 10, mc.NONE)
    assert (it, conv, brk, rel) == (0, True, 0, 0.0) and not x.any()
    # NOT_FINITE: an inf in b, x left at the guess
    bad = b.copy()
    bad[5] = np.inf
    x, it, conv, brk, rel = mc.restate(n, rp, ci, va, bad, x0, 1e-6, 10, mc.JACOBI)
    assert (it, conv, brk) == (0, False, mc.NOT_FINITE) and np.array_equal(x, x0)
    # SINGULAR: [[0, 0], [0, 1]] with b = e_1: A v = 0, alpha = 0, beta = 0, gamma = 0
    rp2, ci2, va2 = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([0.0, 1.0], np.float32)
    x, it, conv, brk, rel = mc.restate(2, rp2, ci2, va2, np.array([1, 0], np.float32), np.zeros(2), 1e-6, 10, mc.NONE)
    assert (it, conv, brk, rel) == (0, False, mc.SINGULAR, 1.0) and not x.any()
    # PRECONDITIONER: a negative definite M
    x, it, conv, brk, rel = mc.restate(n, rp, ci, va, b, x0, 1e-6, 10, apply_m=lambda u: -u)
    assert (it, conv, brk) == (0, False, mc.PRECONDITIONER) and np.array_equal(x, x0)
    # the shift equals csr_add's matrix: the shifted solve and the solve of the shifted matrix walk the same path
    base = mc.spd.random_spd(500, 7, seed=3)
    a = mc.restate(n, *base[1:], b, np.zeros(n), 0.0, 8, mc.JACOBI, shift=8.0)
    c = mc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, 8, mc.JACOBI)
    assert abs(a[4] - c[4]) <= 1e-5 * c[4]


# ------------------------------------------------------------------------------------------ the exact families
def _exact_sizes():
    """the sizes test_gpu_minres_exact.py runs, the tiled one among them"""
    return [(n, 1) for n in ed.TRIP_SIZES] + [(n, L) for L, n in ed.LANE_SIZES.items()]


@pytest.mark.parametrize("family", mc.EXACT_FAMILIES)
def test_exact_families_are_exact(family):
    """Every vector entry and every scalar of both steps is a dyadic rational that fp32 holds (prove_exact asserts it
    in integer / Fraction arithmetic), no row sum can round in any order, and restate() returns the proven values to
    the bit.  At the first two sizes of every kind; the larger ones are the same construction."""
    sizes = [(257, 1), (1201, 1), (1201, 2), (2049, 4), (2049, 8), (3001, 16), (4001, 32), (4001, 64)]
    for n, L in sizes:
        system = mc.exact_system(family, n, L)
        rp, ci, va = system["rp"], system["ci"], system["va"]
        rows = np.repeat(np.arange(n), np.diff(rp))
        # symmetric: the multiset of (row, col, value) equals that of (col, row, value)
        fwd = np.lexsort((va, ci, rows))
        bwd = np.lexsort((va, rows, ci))
        assert np.array_equal(rows[fwd], ci[bwd]) and np.array_equal(ci[fwd], rows[bwd]) and \
            np.array_equal(va[fwd], va[bwd]), (family, n, L)
        support = int(np.count_nonzero(system["b"]))
        assert support >= 4 and support & (support - 1) == 0 and (support.bit_length() - 1) % 2 == 0
        for kind in mc.exact_preconditioners(family):
            for steps in (1, 2):
                x, it, conv, rel = mc.prove_exact(system, kind, steps)
                rx, rit, rconv, rbrk, rrel = mc.exact_reference(system, kind, steps)
                assert (it, conv, rbrk) == (rit, rconv, 0), (family, n, L, kind, steps)
                assert np.array_equal(x.view(np.uint32), rx.view(np.uint32)), (family, n, L, kind, steps)
                assert np.float32(rel) == np.float32(rrel)
                if family == "eigen":
                    assert (it, conv, rel) == (1, True, 0.0)
                    assert np.array_equal(x, system["b"] / np.float32(mc.PAIR_C))
                else:
                    assert (it, conv, rel) == ((1, False, 1.0) if steps == 1 else (2, True, 0.0))
                    if steps == 1:
                        assert not x.any()
                if conv:
                    assert mc.true_residual(rp, ci, va, system["b"], x, system["shift"]) == 0.0


def test_exact_sizes_reach_every_lane_count_and_a_second_trip():
    sizes = _exact_sizes()
    assert sorted({L for _, L in sizes}) == list(ed.LANES)
    assert max(n for n, L in sizes if L == 1) > ed.row_trip(1) and ed.TILED_TRIP_SIZE in [n for n, _ in sizes]
    for L, n in ed.LANE_SIZES.items():
        assert n > ed.row_trip(L)
