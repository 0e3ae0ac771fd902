"""CPU tier of the exact-arithmetic tests: every matrix tests/test_gpu_lane_sweep.py runs is generated here and
proved exact without a GPU.  Per matrix: the sum_j |a_ij| |x_j| < 2^24 bound holds, the lane rule gives the L its
name claims, and the CPU oracle (CPU order, fp32) and the library's own spmv_cpu_csr equal the int64 reference
bit for bit: the data are order-independent, so the GPU tests may demand bit equality from every kernel."""
import importlib
import math

import numpy as np
import pytest

import exact_data as ed
import gmres_cases as gc


def host_library_y(spmv, rows, num_cols, rp, ci, va, x):
    A = spmv.csr_from_arrays(rows, num_cols, rp, ci, va)
    try:
        return spmv.spmv_cpu_csr(A, x)
    finally:
        spmv.csr_destroy(A)


def prove_exact(spmv, oracle, num_cols, rp, ci, va, x):
    ed.check_exact(rp, ci, va, x)
    want = ed.exact_reference(rp, ci, va, x)
    np.testing.assert_array_equal(oracle.spmv_csr(rp, ci, va, x), want)
    np.testing.assert_array_equal(host_library_y(spmv, len(rp) - 1, num_cols, rp, ci, va, x), want)
    return want


def test_lane_rule_restatement_at_every_threshold():
    for L in ed.LANES:
        for rows in (1, 7, 1003, 4099):
            assert ed.lanes_for(4 * L * rows, rows) == L
            assert ed.lanes_for(4 * L * rows + 1, rows) == min(2 * L, 64)
    assert ed.lanes_for(0, 5) == 1 and ed.lanes_for(10**7, 3) == 64


def test_exact_csr_data_and_its_bound():
    rng = np.random.default_rng(1)
    rp, ci, va, x = ed.exact_csr(rng, [3, 0, 32767, 5], 1000)
    assert va.dtype == x.dtype == np.float32 and ci.dtype == rp.dtype == np.int32
    assert np.all(va != 0) and np.abs(va).max() <= 8 and np.abs(x).max() <= 64
    assert (va < 0).any() and (va > 0).any() and (x < 0).any() and np.unique(x).size > 100
    assert np.unique(ci[rp[2]:rp[3]]).size < 32767                  # repeats allowed
    assert np.any(np.diff(ci[rp[2]:rp[3]]) < 0)                     # unsorted
    with pytest.raises(AssertionError):                             # a row the defaults cannot keep exact
        ed.check_exact(np.array([0, 32768]), np.zeros(32768, np.int32), np.full(32768, 8, np.float32),
                       np.full(10, 64, np.float32))
    ed.check_exact(np.array([0, 32767]), np.zeros(32767, np.int32), np.full(32767, 8, np.float32),
                   np.full(10, 64, np.float32))
    ed.exact_csr(rng, [40000], 10, vmax=4, xmax=64)                 # smaller values: longer rows


@pytest.mark.parametrize("rows,num,den", [(1003, 4, 1), (1003, 2 * 1003 + 1, 1003), (1003, 501, 1003), (300, 7, 2),
                                          (4099, 200, 1)])
def test_lens_for_average(rows, num, den):
    lens = ed.lens_for_average(rows, num, den, np.random.default_rng(rows))
    assert lens.size == rows and lens.min() == 0 and int(lens.sum()) * den == rows * num
    assert (lens == 0).sum() >= rows // 11 and lens[-1] == 0
    assert lens.max() >= 3 * num / den and (num < den or (lens % 4 != 0).sum() > rows // 4)


@pytest.mark.parametrize("name", ed.SWEEP_NAMES)
def test_sweep_matrix_is_exact_and_lands_on_its_lanes(spmv, oracle, name):
    L, rp, ci, va, x = ed.sweep_matrix(name)
    rows, nnz = ed.SWEEP_ROWS, int(rp[-1])
    assert len(rp) - 1 == rows and rows % 4 != 0                    # idle row slots in the last workgroup at every L
    assert nnz == dict((c[0], c[2]) for c in ed.sweep_counts(rows))[name]
    assert ed.lanes_for(nnz, rows) == L == int(name[1:].split("_")[0])
    if name.endswith("_top") and L < 64:
        assert nnz == 4 * L * rows and ed.lanes_for(nnz + 1, rows) == 2 * L
    if name.endswith("_low") and L > 1:
        assert nnz == 2 * L * rows + 1 and ed.lanes_for(nnz - 1, rows) == L // 2
    prove_exact(spmv, oracle, ed.SWEEP_COLS, rp, ci, va, x)
    # the multi-vector sweep's X: every column under the same bound, every column's oracle result exact
    X = ed.exact_x_matrix(np.random.default_rng(5), ed.SWEEP_COLS, 19)
    ed.check_exact(rp, ci, va, X)
    for j in (0, 18):
        col = np.ascontiguousarray(X[:, j])
        np.testing.assert_array_equal(oracle.spmv_csr(rp, ci, va, col), ed.exact_reference(rp, ci, va, col))


@pytest.mark.parametrize("name", ed.SWEEP_NAMES)
def test_ldsx_matrix_is_exact_and_meets_the_x_in_lds_conditions(spmv, oracle, name):
    L, num_cols, rp, ci, va, x = ed.ldsx_matrix(name)
    rows, nnz = len(rp) - 1, int(rp[-1])
    assert ed.lanes_for(nnz, rows) == L
    # vector_ldsx_grid (csrc/kernels.hip): rows >= 4096, columns <= 32768, min(256, nnz * 8 / (8 * 4 * cols)) >= 64;
    # and below the tiled engine's column minimum (32769), so use_texture keeps the direct kernel
    assert rows >= 4096 and 0 < num_cols <= 32768 and (nnz * 8) // (8 * 4 * num_cols) >= 64
    prove_exact(spmv, oracle, num_cols, rp, ci, va, x)


def test_ldsx_catalogue_takes_both_branches_of_the_copy_loop():
    cols = [ed.ldsx_matrix(name)[1] for name in ed.SWEEP_NAMES]
    assert any(c % 4 == 0 for c in cols) and any(c % 4 != 0 for c in cols)


def merge_items(rp):
    """Merge item index (0-based) of every row's end: the row's entries come first, then its end."""
    rp = np.asarray(rp, np.int64)
    return rp[1:] + np.arange(rp.size - 1)


@pytest.mark.parametrize("name", ed.MERGE_CUT_NAMES)
def test_merge_cut_matrix_is_exact_and_sits_where_its_name_says(spmv, oracle, name):
    rp, ci, va, x = ed.merge_cut_matrix(name)
    T = ed.MERGE_TILE
    rows, nnz = len(rp) - 1, int(rp[-1])
    ends, lens = merge_items(rp), np.diff(rp.astype(np.int64))
    total = rows + nnz
    if name.startswith("total_"):
        assert total == {"T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[name[6:]]
    elif name.startswith("row_end_"):
        assert {"T-2": T - 2, "T-1": T - 1, "T": T}[name[8:]] in ends and total > 2 * T
    elif name.endswith("over_four_tiles"):
        long_rows = np.flatnonzero(lens > 2 * T)
        assert long_rows.size == (2 if name.startswith("two") else 1) and lens[0:long_rows[0]].max() < 9
        for r in long_rows:              # first entry in tile t, row end in tile t + 3: three tiles carry into it
            assert ends[r] // T - (ends[r] - lens[r]) // T == 3
        assert np.all(np.diff(long_rows) == 1) and rows - long_rows[-1] > 100
    elif name.startswith("empty_run"):
        empty = np.flatnonzero(lens == 0)
        run = np.split(empty, np.flatnonzero(np.diff(empty) > 1) + 1)
        longest = max(run, key=len)
        assert len(longest) >= 2000 > T
        assert (longest[-1] == rows - 1) == name.endswith("at_the_end")
    else:
        r = int(np.flatnonzero(ends == 2 * T)[0])
        assert (ends[r] - lens[r]) // T == 0                      # its first entry is in tile 0
    prove_exact(spmv, oracle, ed.MERGE_CUT_COLS, rp, ci, va, x)
    X = ed.exact_x_matrix(np.random.default_rng(6), ed.MERGE_CUT_COLS, 20)
    ed.check_exact(rp, ci, va, X)


@pytest.mark.parametrize("symmetric", [True, False], ids=["spd", "nonsym"])
@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_solver_system_is_exact_dominant_and_lands_on_its_lanes(spmv, oracle, name, symmetric):
    L, n, rp, ci, va, x_star, b = ed.solver_system(name, symmetric)
    nnz = int(rp[-1])
    assert n <= 2000 and ed.lanes_for(nnz, n) == L == int(name[1:].split("_")[0])
    if name.endswith("_top") and L < 64:
        assert nnz == 4 * L * n
    if name.endswith("_low") and L > 1:
        assert nnz == 2 * L * n + 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    dense = np.zeros((n, n), np.int64)
    np.add.at(dense, (rows, ci), va.astype(np.int64))
    off = np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))
    assert np.all(np.diag(dense) > off)                             # strictly diagonally dominant, positive diagonal
    assert np.array_equal(dense, dense.T) == symmetric
    for vec in (x_star, b):
        want = prove_exact(spmv, oracle, n, rp, ci, va, vec)
        np.testing.assert_array_equal(want.astype(np.int64), dense @ vec.astype(np.int64))
    # what the one-step CG test predicts from: r.z = b.b and p.q = b.(A b) are integers below 2^53
    q = dense @ b.astype(np.int64)
    assert 0 < int(b.astype(np.int64) @ q) < 2**53


@pytest.mark.parametrize("name,L,k", ed.PAGERANK_CASES)
def test_pagerank_graph_lands_on_its_lanes(spmv, name, L, k):
    graph = importlib.import_module("test_gpu_pagerank").graph
    rp, ci, va = ed.pagerank_graph(spmv, graph, k, 40 + k)
    assert np.all(np.isfinite(va)) and np.all(va > 0)
    assert ed.lanes_for(int(rp[-1]), ed.PAGERANK_N) == L
    assert not np.isin(ci, np.array(ed.PAGERANK_DANGLING)).any()


def test_ell_cases_are_exact(oracle):
    for width, rows, rp, ci, va, x in ed.ell_cases():
        ed.check_exact(rp, ci, va, x)
        kk, ecols, evals = oracle.ell_from_csr(rp, ci, va)
        assert kk == width and len(rp) - 1 == rows
        np.testing.assert_array_equal(oracle.spmv_ell(rows, kk, ecols, evals, x), ed.exact_reference(rp, ci, va, x))
    shapes = {(w, r % 4) for w, r, *_ in ed.ell_cases()}
    assert shapes == {(w, m) for w in range(1, 10) for m in range(4)}


# ------------------------------------------------------------------------------------------ dyadic PageRank
def test_dyadic_prover_on_a_graph_small_enough_to_do_by_hand():
    """Two nodes linking to each other and a dangling third, n padded to 4 with a second dangling node, d = 0.5:
    A r = (1/4, 1/4, 0, 0), s = 1/2, r_new = 1/8 + 1/16 + 1/8 for the first two, 1/16 + 1/8 for the others."""
    rp, ci, va = np.array([0, 1, 2, 2, 2], np.int32), np.array([1, 0], np.int32), np.ones(2, np.float32)
    ranks, residual = ed.dyadic_pagerank(rp, ci, va, 4, 0.5, 1)
    np.testing.assert_array_equal(ranks, np.array([5, 5, 3, 3], np.float32) / 16)
    assert residual == np.sqrt(4 * (1 / 16) ** 2) and ed.exact_steps(rp, ci, va, 4, 0.5) >= 1
    # a value that needs more than 24 bits in the first step is noticed: 2^24 + 1 links of weight 1 cannot be built
    # here, so shrink the budget instead: one rank of 25 significant bits fails the representability test
    assert ed._fits_float32(np.array([(1 << 24) - 1, 1 << 40, 0, 3 << 50])) and not ed._fits_float32([(1 << 24) + 1])


@pytest.mark.parametrize("name", [c[0] for c in ed.DYADIC_DIRECT] + list(ed.DYADIC_TILED))
def test_dyadic_case_is_exact_and_restates_the_oracle(oracle, name):
    """exact_steps >= 1 (>= 3 without dangling nodes): a case with 0 is a construction error.  The integer PageRank
    agrees with the oracle's fp64-sum loop to 1e-6 relative at the same step count (a restatement check)."""
    n, rp, ci, va, steps, ranks, residual = ed.dyadic_case(name)
    lens = np.diff(rp.astype(np.int64))
    dangling = np.flatnonzero(np.bincount(ci, minlength=n) == 0)
    assert n & (n - 1) == 0 and (lens == 0).sum() >= n // 14 and np.all(np.frexp(va)[0] == 0.5)
    for r in np.flatnonzero(lens > 1)[:200]:
        assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)                       # distinct ascending columns
    if name in ed.DYADIC_TILED:
        _, W, R, dangling_count, _, _, wanted = ed.DYADIC_TILED[name]
        assert dangling.size == dangling_count and steps >= wanted
        assert (lens > ed.default_long_row(-(-n // W))).sum() >= 2              # hubs beyond the long-row limit
    else:
        L = next(c[1] for c in ed.DYADIC_DIRECT if c[0] == name)
        assert ed.lanes_for(int(rp[-1]), n) == L and dangling.size == len(ed.DYADIC_DIRECT_DANGLING)
    assert steps >= 1, "not one exact step: the case is built wrongly"
    assert ranks.dtype == np.float32 and abs(float(ranks.astype(np.float64).sum()) - 1.0) == 0.0
    want, iters, res, _ = oracle.pagerank(rp, ci, va, num_cols=n, damping=ed.DYADIC_DAMPING, tolerance=0.0,
                                          max_iterations=steps, wide_sums=True)
    assert iters == steps
    assert float(np.max(np.abs(ranks.astype(np.float64) - want) / want)) <= 1e-6
    assert abs(res - residual) <= 1e-5 * residual


SOURCE_NAMES = list(ed.DYADIC_SOURCES) + [c[0] for c in ed.DYADIC_SOURCE_DIRECT]


@pytest.mark.parametrize("name", SOURCE_NAMES)
def test_source_only_dangling_cases_stay_exact_beyond_the_first_step(name):
    """The cases whose dangling nodes are source-only nodes: at least TWO exact steps with dangling nodes present
    (so the mass the device accumulates in step 1 enters step 2 under a bit-exact comparison), the ranks summing to
    exactly 1 after EVERY step, all dangling nodes without in-links, the hubs beyond the long-row limit at the strip
    count of the unsharded matrix (the sharded layouts, whose padded vectors are wider, are checked in
    test_hubs_stay_long_rows_in_every_sharded_layout)."""
    n, rp, ci, va, steps, ranks, residual = ed.dyadic_case(name)
    lens = np.diff(rp.astype(np.int64))
    dangling = np.flatnonzero(np.bincount(ci, minlength=n) == 0)
    assert dangling.size == 1 << 12 and np.all(lens[dangling] == 0) and np.all(dangling % 13 == 5)
    assert steps >= 2 and steps == ed.exact_steps(rp, ci, va, n, ed.DYADIC_DAMPING)
    trajectory = ed.dyadic_trajectory(rp, ci, va, n, ed.DYADIC_DAMPING, steps)
    assert len(trajectory) == steps
    for r, res in trajectory:
        assert r.dtype == np.float32 and float(r.astype(np.float64).sum()) == 1.0 and res > 0
        assert np.unique(r[dangling]).size == 1                                # one short rank for all of them
    np.testing.assert_array_equal(trajectory[-1][0], ranks)
    assert trajectory[-1][1] == residual
    w = ed.DYADIC_TILED[name][1] if name in ed.DYADIC_TILED else ed.SHARD_W
    assert (lens > ed.default_long_row(-(-n // w))).sum() >= 2
    if name.startswith("sources_L"):
        L = next(c[1] for c in ed.DYADIC_SOURCE_DIRECT if c[0] == name)
        assert ed.lanes_for(int(rp[-1]), n) == L


def test_some_source_only_case_has_three_exact_steps_and_the_sharded_one_does():
    assert ed.dyadic_case(ed.SHARDED_CASE)[4] >= 3
    assert sum(ed.dyadic_case(name)[4] >= 3 for name in SOURCE_NAMES) >= 1
    assert ed.DYADIC_TILED[ed.SHARDED_CASE][1:3] == (ed.SHARD_W, ed.SHARD_R)


def test_existing_dyadic_cases_keep_their_arrays():
    """dyadic_case grew new branches; the cases that were there draw the same graphs (checksums of the arrays as they
    were before the source-only cases were added)."""
    import zlib
    want = {"L1": (4763, 2663063358), "L2": (12272, 3988500013), "L4": (24464, 1090606460), "L8": (48992, 968007382),
            "L16": (98016, 3587197183), "L32": (194752, 631239565), "L64": (391808, 2736269738),
            "n16_4096x64_dangling_fold": (483458, 3412015588), "n16_8192x1024_closed_fold": (98247, 1151884295),
            "n16_16384x9984_dangling_stream": (484422, 316532757), "n18_4096x64_closed_stream": (393584, 3752300066),
            "n18_8192x1024_dangling_fold": (1939084, 683648082), "n18_16384x9984_closed_fold": (392861, 3523887001),
            "n16_8192x1024_closed_switch_after_1": (98494, 4166476643)}
    for name, (nnz, crc) in want.items():
        _, rp, ci, va, *_ = ed.dyadic_case(name)
        assert (int(rp[-1]), zlib.crc32(rp.tobytes() + ci.tobytes() + va.tobytes())) == (nnz, crc), name


def sharded_graph():
    n, rp, ci, va, steps, _, _ = ed.dyadic_case(ed.SHARDED_CASE)
    dangling = np.flatnonzero(np.bincount(ci, minlength=n) == 0)
    return n, rp, ci, va, dangling, ed.DYADIC_SOURCES[ed.SHARDED_CASE](n)


def assert_spread(bounds, dangling, min_rows=100):
    counts = ed.dangling_per_rank(bounds, dangling)
    big = np.diff(np.asarray(bounds)) > min_rows
    assert (counts[big] > 0).all() and np.unique(counts[big]).size == int(big.sum()), (bounds, counts)
    return counts


def test_every_rank_of_every_sharded_case_owns_dangling_nodes_of_a_different_mass(spmv):
    """All dangling nodes carry the same rank, so a rank's partial mass is proportional to the number it owns: the
    counts are positive and pairwise different for every world size under both cuts (Layout's and the native
    loop's), for the chunk-major worlds, and among the shards of more than 100 rows of every explicit cut."""
    import ctypes
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    n, rp, ci, va, dangling, hubs = sharded_graph()
    for world in ed.SHARD_WORLDS:
        lay = prd.Layout(n, world)
        np.testing.assert_array_equal(lay.bounds, ed.equal_row_bounds(n, world))
        for bounds in (lay.bounds, prd.Layout.equal_nnz_bounds(rp, world)):
            counts = assert_spread(bounds, dangling)
            assert counts.size == world and counts.min() > 0 and np.unique(counts).size == world
        native = np.zeros(world + 1, np.int32)
        assert spmv.lib().spmv_c_pagerank_shard_bounds(rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, world,
                                                       native.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
        # the two partitions are separate code (csrc/pagerank_multi.cpp, pagerank_dist.py): they must cut alike
        np.testing.assert_array_equal(native, prd.Layout.equal_nnz_bounds(rp, world))
    for chunks in ed.SHARD_CHUNKS:
        world, bounds = ed.chunk_world(n, chunks)
        counts = assert_spread(prd.Layout(n, world, 0, bounds=bounds).bounds, dangling)
        assert counts.size == world and counts.min() > 0
    for name, bounds in ed.shard_cut_edges(n, hubs[0][0]).items():
        counts = assert_spread(bounds, dangling)
        assert (counts > 0).sum() >= 2 or name == "one_empty_row", (name, counts)


def test_hubs_stay_long_rows_in_every_sharded_layout():
    """The long-row limit (8 per strip) grows with the strip count, and a shard's matrix is as wide as the PADDED
    vector, world * (longest shard + tail) and more in the chunk-major layouts.  Both hubs exceed the limit under the
    equal-row and equal-nnz cuts of every world size; the uneven explicit cuts and the chunk-major layouts pad up to
    48 strips of 4096 columns (limit 384), where only the 700-entry hub does: the GPU tests assert what holds
    everywhere, at least one long row."""
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    n, rp, ci, va, dangling, hubs = sharded_graph()
    lengths = [length for _, length in hubs]
    even = [prd.Layout(n, 1, 0, exchange=True)]
    for world in ed.SHARD_WORLDS:
        even += [prd.Layout(n, world), prd.Layout(n, world, 0, bounds=prd.Layout.equal_nnz_bounds(rp, world))]
    assert min(lengths) > ed.default_long_row(max(-(-lay.padded // ed.SHARD_W) for lay in even))
    other = [prd.Layout(n, len(b) - 1, 0, bounds=b) for b in ed.shard_cut_edges(n, hubs[0][0]).values()]
    for chunks in ed.SHARD_CHUNKS:
        world, bounds = ed.chunk_world(n, chunks)
        other += [prd.Layout(n, world, 0, bounds=bounds, chunks=chunks, align=a) for a in ed.SHARD_ALIGNS]
    most = max(-(-lay.padded // ed.SHARD_W) for lay in other)
    assert 40 <= most <= 48 and max(lengths) > ed.default_long_row(most)


def test_sharded_cut_edges_are_what_their_names_say():
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    n, rp, ci, va, dangling, hubs = sharded_graph()
    lens = np.diff(rp.astype(np.int64))
    hub = hubs[0][0]
    limit = ed.default_long_row(-(-n // ed.SHARD_W) + 1)
    assert lens[hub] == hubs[0][1] > limit and lens[n - 1] == hubs[1][1] > limit
    cuts = ed.shard_cut_edges(n, hub)
    rows = {name: np.diff(b) for name, b in cuts.items()}
    assert rows["empty_first"][0] == 0 and rows["empty_middle"][1] == 0 and rows["empty_last"][2] == 0
    b = cuts["one_empty_row"]
    assert rows["one_empty_row"][1] == 1 and rp[b[2]] - rp[b[1]] == 0
    assert rows["hub_alone"][1] == 1 and cuts["hub_alone"][1] == hub
    assert rows["last_hub_alone"][2] == 1 and cuts["last_hub_alone"][2] == n - 1
    assert cuts["cut_before_hub"][1] == hub and cuts["cut_after_hub"][1] == hub + 1
    assert rows["odd_lengths"].max() % 2 == 1
    lay = prd.Layout(n, 3, 0, bounds=cuts["odd_lengths"])
    assert lay.shard_len == rows["odd_lengths"].max() + 1 and lay.piece == lay.shard_len + prd.TAIL
    for world in (3, 5):                                     # equal rows: world * shard_len overshoots n
        lay = prd.Layout(n, world)
        assert world * lay.shard_len > n and np.diff(lay.bounds)[-1] < lay.shard_len


def test_chunk_major_cases_put_block_boundaries_where_they_claim():
    """align = W and 2 W: every block boundary is a strip boundary; align = 1000: some boundary falls inside a strip
    (pr_expand must round cols_ready / strip_cols down).  The tail sits in the last piece; at 7 chunks (and at a
    wide align) the short shards' last pieces hold no rows; positions() is a bijection onto distinct slots that
    miss every tail."""
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    n = sharded_graph()[0]
    W = ed.SHARD_W
    assert [a % W == 0 for a in ed.SHARD_ALIGNS] == [True, True, False] and W % ed.SHARD_ALIGNS[2] != 0
    empty_pieces = 0
    for chunks in ed.SHARD_CHUNKS:
        world, bounds = ed.chunk_world(n, chunks)
        for align in ed.SHARD_ALIGNS:
            lays = [prd.Layout(n, world, r, bounds=bounds, chunks=chunks, align=align) for r in range(world)]
            lay = lays[0]
            assert lay.chunks == chunks and lay.piece % align == 0 and lay.padded == chunks * world * lay.piece
            inside = [c for c in range(1, chunks) if (c * lay.block) % W]
            assert bool(inside) == (align % W != 0)
            pos = lay.positions()
            assert np.unique(pos).size == n and pos.max() < lay.padded
            for r, l in enumerate(lays):
                tail = lay.tail_slice(r)
                assert tail.stop == (chunks - 1) * lay.block + (r + 1) * lay.piece
                assert not np.isin(np.arange(tail.start, tail.stop), pos).any()
                assert l.local_rows <= lay.shard_len
                np.testing.assert_array_equal(l.local_positions(), pos[l.row_begin:l.row_end])
                empty_pieces += sum(c * lay.piece >= l.local_rows for c in range(chunks))
    assert empty_pieces > 10


def cpu_world(oracle, world, **layout):
    """shard_sim.Sim over the sharded graph with the CPU double of the shard engine (test_distributed_gloo.OracleEngine:
    fp32 update, double partial sums, the same padded layout) in place of HipEngine."""
    import torch
    import shard_sim
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    class double(importlib.import_module("test_distributed_gloo").OracleEngine):
        """The promise of expand() checked on the bits: the vectors' padding holds a NaN pattern here."""

        def expand(self, r_old, cols_ready):
            assert 0 < cols_ready <= self.layout.padded and cols_ready % self.layout.block == 0
            self.seen = getattr(self, "seen", []) + [(cols_ready, r_old[:cols_ready].view(torch.int32).clone())]

        def step(self, r_old, r_new, damping, sums_out=None):
            for cols_ready, seen in getattr(self, "seen", []):
                assert torch.equal(r_old[:cols_ready].view(torch.int32), seen), "columns changed after expand()"
            self.seen = []
            return super().step(r_old, r_new, damping, sums_out)

    n, rp, ci, va, _, _ = sharded_graph()
    return shard_sim.Sim(None, prd, torch, rp, ci, va, n, world,
                         make_engine=lambda lrp, lci, lva, lay: double(oracle, lrp, lci, lva, lay), **layout)


def cpu_worlds():
    n, hub = 1 << 16, (1 << 16) // 3
    cuts = ed.shard_cut_edges(n, hub)
    yield "world3_rows_gather", 3, {}, "gather", "blocks"
    yield "world8_rows_sums", 8, {}, "sums", "blocks"
    yield "world1_exchange", 1, dict(exchange=True), "gather", "blocks"
    for name in ("empty_middle", "empty_last", "one_empty_row", "hub_alone", "odd_lengths"):
        yield name, len(cuts[name]) - 1, dict(bounds=cuts[name]), "gather", "blocks"
    for chunks, align, head_start in ((2, 4096, "blocks"), (3, 1000, "twice"), (7, 8192, "blocks"), (4, 1000, "never")):
        world, bounds = ed.chunk_world(n, chunks)
        yield "chunks%d_align%d" % (chunks, align), world, dict(bounds=bounds, chunks=chunks, align=align), "gather", head_start


@pytest.mark.parametrize("what,world,layout,mode,head_start", list(cpu_worlds()), ids=[c[0] for c in cpu_worlds()])
def test_shard_simulator_and_layout_reproduce_the_prover_on_the_cpu(oracle, what, world, layout, mode, head_start):
    """The simulator the GPU tests use (tests/shard_sim.py: cutting, renumbering, exchange by pieces, tails, commit
    forms, padding sentinel, the per-step checks) with a CPU engine: every rank's vector equals the integer prover's
    bit for bit after every step.  On dyadic data the CPU double's row sums are exact in its order as in any other,
    so this holds Layout, the catalogue and the simulator themselves to the bits before a GPU is involved; a failure
    of the GPU tests is then the engine's."""
    n, rp, ci, va, dangling, _ = sharded_graph()
    steps = ed.dyadic_case(ed.SHARDED_CASE)[4]
    trajectory = ed.dyadic_trajectory(rp, ci, va, n, ed.DYADIC_DAMPING, steps)
    sim = cpu_world(oracle, world, **layout)
    assert all(sp.num_dangling == dangling.size for sp in sim.loops)

    def same_bits(_, got, want, where):
        np.testing.assert_array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32), err_msg=str(where))

    try:
        for k in range(steps):
            sim.step(k, ed.DYADIC_DAMPING, 0.0, mode=mode, head_start=head_start)
            sim.check(k, trajectory[k][0], trajectory[k][1], same_bits, what)
    finally:
        sim.close()


# ------------------------------------------------------------------------------------------ plan geometry
@pytest.mark.parametrize("name", ed.GEOMETRY_NAMES)
def test_geometry_case_is_exact_and_the_host_logic_gives_its_shape(spmv, oracle, monkeypatch, name):
    case, rp, ci, va, x = ed.geometry_matrix(name)
    rows, cols, nnz = case["rows"], case["cols"], int(rp[-1])
    assert len(rp) - 1 == rows and int(ci.max()) < cols and nnz > 0
    prove_exact(spmv, oracle, cols, rp, ci, va, x)
    monkeypatch.setenv("SPMV_DEBUG", case["debug"])
    assert spmv.tiled_shape(rows, cols, nnz) == (True, case["W"], case["R"])
    monkeypatch.delenv("SPMV_DEBUG")
    assert not spmv.tiled_shape(rows, cols, nnz)[0]                             # only the override lets it in
    # one value per column exactly when the case says the plan folds
    order = np.argsort(ci, kind="stable")
    same_column = ci[order][1:] == ci[order][:-1]
    differs = bool(np.any(same_column & (va[order][1:] != va[order][:-1])))
    assert differs != case["fold"] and same_column.any()
    lens = np.diff(rp.astype(np.int64))
    limit = ed.LONG_LIMIT if name.startswith("long_rows") else ed.default_long_row(case["strips"])
    assert int((lens > limit).sum()) == case["long_rows"]
    local = ci % case["W"]
    if name.startswith(("strip_", "tile_")):
        assert (local == 0).any() and (local == case["W"] - 1).any() and (ci == cols - 1).any() and lens[-1] > 0
        assert np.unique(ci // case["W"]).size == case["strips"]                # entries in the last, partial strip too


def test_geometry_catalogue_covers_what_it_claims():
    cases = ed.GEOMETRY_CASES.values()
    assert {(c["W"], c["fold"]) for c in cases} == {(w, f) for w in (4096, 8192, 16384, 32768) for f in (False, True)}
    assert {c["R"] for c in cases} == {64, 128, 1024, 4800, 9984}
    assert {c["cols"] % c["W"] for c in cases if c["name"].startswith("strip_")} >= {0, 1}
    assert all(c["rows"] <= 20000 and c["strips"] <= 64 for c in cases)
    # the row-delta case: gaps of exactly 1, 254, 255, 256, 509, 510, 511 and 9983 rows inside one cell
    case, rp, ci, _, _ = ed.geometry_matrix("row_deltas_stream")
    rows_of = np.repeat(np.arange(case["rows"]), np.diff(rp))
    for tile in (0, 1):
        in_tile = rows_of // 9984 == tile
        gaps = set(np.diff(np.unique(rows_of[in_tile & (ci < 4096)])))
        assert gaps == {1, 254, 255, 256, 509, 510, 511}, gaps
        assert set(np.diff(np.unique(rows_of[in_tile & (ci // 4096 == 1)]))) == {9983 - 7 * tile}   # 39 skip markers
    assert set(rows_of[ci // 4096 == 2]) == {9983}                              # first entry in the tile's last row
    case, rp, ci, _, _ = ed.geometry_matrix("items_1024_stream")
    assert tuple(np.bincount(ci // 4096, minlength=6)) == ed.ITEM_STRIP_ENTRIES
    rows_of = np.repeat(np.arange(case["rows"]), np.diff(rp))
    for strip in range(6):                                                      # consecutive rows: no skip markers
        r = np.unique(rows_of[ci // 4096 == strip])
        assert r.size == 0 or (r[0] == 0 and np.all(np.diff(r) == 1))


# ------------------------------------------------------------------------------------------ array-view catalogue
def test_view_catalogue_picks_what_it_claims():
    names = ed.VIEW_NAMES
    assert [n for n in names if n.startswith("sweep:")] == ["sweep:L1_low", "sweep:L4_top", "sweep:L16_low", "sweep:L64_top"]
    assert sum(n.startswith("ldsx:") for n in names) == 1 and sum(n.startswith("merge:") for n in names) == 2
    assert "tiled:%dx%d" % min(ed.ENTRY_POINT_GEOMETRIES) in names
    T = ed.MERGE_TILE
    ends = {n: merge_items(ed.view_matrix(n)["rp"]) for n in names if n.startswith("merge:")}
    assert T - 1 in ends["merge:row_end_T-1"]                                   # tile 0 ends on a row end
    long_row = ends["merge:row_over_four_tiles"]
    assert not np.any((long_row >= T) & (long_row < 3 * T))                     # tiles 1 and 2: inside one row
    # every array meets every residue; cols and vals part ways
    for k in range(3):
        assert {t[k] for t in ed.VIEW_OFFSETS} == {0, 1, 2, 3}
    assert any(t[1] != t[2] for t in ed.VIEW_OFFSETS)


@pytest.mark.parametrize("name", ed.VIEW_NAMES)
def test_view_matrix_is_exact_and_no_stray_entry_can_hide(spmv, oracle, monkeypatch, name):
    """Per member: exact under the non-zero x; one stray entry of any kind added to any row changes the int64
    reference (by at least 2^22 when it carries the value or the x poison) while every true row sum stays below
    2^24; the lane rule (and for the tiled member the shape rule) lands where the GPU test expects."""
    m = ed.view_matrix(name)
    rp, ci, va, x, num_cols, rows = m["rp"], m["ci"], m["va"], m["x"], m["num_cols"], m["rows"]
    nnz = int(rp[-1])
    want = prove_exact(spmv, oracle, num_cols, rp, ci, va, x).astype(np.int64)
    assert np.all(x != 0) and np.all(va != 0) and np.abs(x).min() >= 1 and np.abs(va).min() >= 1
    assert int(ed.row_abs_sums(rp, ci, va, x).max()) < ed.EXACT_LIMIT
    poison = np.int64(ed.VIEW_POISON)
    assert poison == 1 << 22 and np.float32(ed.VIEW_POISON) == ed.VIEW_POISON
    x64, v64 = x.astype(np.int64), va.astype(np.int64)
    poison_col = num_cols - 1
    # the stray entry (column, value) a row may pick up: a live neighbour, the column poison with a live or the
    # poison value, a live column with the poison value; and a live entry multiplied by the x poison
    deltas = [v64 * x64[ci], v64 * x64[poison_col], poison * x64[ci], v64 * poison, np.array([poison * x64[poison_col]])]
    for d in deltas:
        assert np.all(d != 0)
    for d in deltas[2:]:
        assert np.abs(d).min() >= 1 << 22
    # spelled out on the reference: appending any one of them to any row changes that row and no other
    stray = np.array([int(d[np.argmin(np.abs(d))]) for d in deltas], np.int64)          # the smallest of each kind
    for s in stray:
        assert np.all(want + s != want)
    lens = np.diff(rp.astype(np.int64))
    for r in (0, int(np.argmax(lens)), int(np.flatnonzero(lens == 0)[0]), rows - 1):    # ... and literally, on four rows
        for col, val in ((poison_col, np.float32(va[0])), (int(ci[0]), np.float32(ed.VIEW_POISON)),
                         (poison_col, np.float32(ed.VIEW_POISON))):
            rp2 = rp.astype(np.int64).copy()
            rp2[r + 1:] += 1
            at = int(rp[r + 1])
            got = ed.row_abs_sums(rp2, np.insert(ci, at, col), np.insert(va, at, val), x)      # bound not asserted: poison
            run = np.concatenate([[0], np.cumsum(np.insert(va, at, val).astype(np.int64) * x64[np.insert(ci, at, col)])])
            y = run[rp2[1:]] - run[rp2[:-1]]
            assert y[r] != want[r] and np.array_equal(np.delete(y, r), np.delete(want, r)) and got[r] > 0
    # row-pointer poison nnz: in range for both entry arrays' extents
    assert 0 <= nnz <= ci.size
    # the kernels the GPU test expects
    assert ed.lanes_for(nnz, rows) == m["L"]
    if m["kind"] == "sweep":
        assert m["L"] == int(m["key"][1:].split("_")[0]) and rows == ed.SWEEP_ROWS
    elif m["kind"] == "ldsx":
        assert rows >= 4096 and 0 < num_cols <= 32768 and (nnz * 8) // (8 * 4 * num_cols) >= 64
        assert num_cols % 4 != 0                                     # the 16-byte copy loop has a tail
    elif m["kind"] == "tiled":
        monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(m["W"], m["R"]))
        assert spmv.tiled_shape(rows, num_cols, nnz) == (True, m["W"], m["R"])
        assert int(lens.max()) <= ed.default_long_row(-(-num_cols // m["W"]))


# ------------------------------------------------------------------------------------------ one-hot Krylov systems
bits = lambda a: np.asarray(a, np.float32).view(np.uint32)
DOTS = {
    "numpy": gc.dot,
    "reversed": lambda a, c: np.float64(np.dot(a.astype(np.float64)[::-1], c.astype(np.float64)[::-1])),
    "correctly rounded": lambda a, c: np.float64(math.fsum((a.astype(np.float64) * c.astype(np.float64)).tolist())),
}


def same_outcome(got, want):
    """every field restate returns, x and the residual on the bits"""
    return (np.array_equal(bits(got[0]), bits(want[0])) and tuple(got[1:5]) == tuple(want[1:5])
            and bits(got[5]) == bits(want[5]))


def onehot_first_cycle(system, columns, precond):
    """The first cycle's Arnoldi steps on the walk positions, spelled out, with the module comment's claims asserted
    per column: h1 is d_(q_j) (JACOBI: d * fp32(1 / d) == 1) at i = j and 0.0 elsewhere, the updated w is one-hot at
    q_j+1 with +-beta, h2 is all 0.0, sqrt(w.w) == |beta| and v_j+1 == +- e_(q_j+1)."""
    m, rp, ci, va, b = ed.onehot_compact(system)
    walk, d, beta = system["walk"], system["d"], system["beta"]
    dinv = (np.float32(1.0) / gc.diag_of(m, rp, ci, va)).astype(np.float32)
    assert np.array_equal(dinv, np.float32(1.0) / d[walk]) and np.array_equal(np.frexp(dinv)[0], np.copysign(0.5, dinv))
    bnorm = np.sqrt(gc.dot(b, b))
    assert bnorm == ed.ONEHOT_RHS
    V = [(b * np.float32(1.0 / bnorm)).astype(np.float32)]
    assert V[0][0] == 1.0 and np.count_nonzero(V[0]) == 1
    for j in range(columns):
        z = (V[j] * dinv).astype(np.float32) if precond == gc.JACOBI else V[j]
        for spmv in (gc.spmv_round_once, gc.spmv_sequential):
            w = spmv(rp, ci, va, z)
            assert np.count_nonzero(w) <= 2
        h1 = [np.float32(gc.dot(v, w)) for v in V]
        expect = np.float32(1.0) if precond == gc.JACOBI else d[walk[j]]
        assert h1[j] == expect and all(h == 0.0 for h in h1[:j])
        for hi, v in zip(h1, V):
            w = gc.fma(-hi, v, w)
        bj = beta[walk[j]] * (dinv[j] if precond == gc.JACOBI else np.float32(1.0))
        if system["empty_column"] == j:
            assert np.count_nonzero(w) == 0                      # the lucky breakdown: h_j+1 == 0
            return j + 1
        assert np.count_nonzero(w) == 1 and w[j + 1] == V[j][j] * bj
        assert all(np.float32(gc.dot(v, w)) == 0.0 for v in V)      # h2
        hn = np.sqrt(gc.dot(w, w))
        assert hn == abs(bj)
        V.append((w * np.float32(1.0 / hn)).astype(np.float32))
        assert np.count_nonzero(V[-1]) == 1 and abs(V[-1][j + 1]) == 1.0
    return columns


@pytest.mark.parametrize("name", ed.ONEHOT_NAMES)
def test_onehot_case_is_what_it_claims(monkeypatch, name):
    """No revisit, the required positions, powers of two, L = 1, the first cycle's exactness claims column by column,
    and the same bits from three dot-product orders and two SpMV orders over the whole run (both preconditioners)."""
    c, s = ed.onehot_case(name)
    n, walk = s["n"], s["walk"]
    assert walk.size == c["max_iterations"] + 1 == np.unique(walk).size and walk[0] == c["p"]
    assert set(c["visits"]) <= set(walk.tolist()) and set(c["chunks"]) <= set((walk // ed.ONEHOT_CHUNK).tolist())
    assert n % 64 != 0 and n % 4 != 0
    nnz = int(s["rp"][-1])
    assert nnz == 2 * n - (c["empty_column"] is not None) and ed.lanes_for(nnz, n) == 1
    assert np.all(np.frexp(np.abs(s["va"]))[0] == 0.5) and np.abs(np.frexp(s["va"])[1] - 1).max() <= 1
    assert np.count_nonzero(s["b"]) == 1 and s["b"][c["p"]] == ed.ONEHOT_RHS
    rows = np.repeat(np.arange(n), np.diff(s["rp"]))
    off = s["ci"] != rows
    assert np.array_equal((s["ci"][off] + c["s"]) % n, rows[off])              # B: column i feeds row (i + s) mod n
    assert np.array_equal(np.sort(s["ci"][~off]), np.arange(n))               # D: every diagonal entry, once
    for precond in (gc.NONE, gc.JACOBI):
        columns = onehot_first_cycle(s, min(c["restart"], c["max_iterations"]), precond)
        outs = {}
        for order, dot in DOTS.items():
            monkeypatch.setattr(gc, "dot", dot)
            outs[order] = ed.gmres_onehot_reference(s, c["restart"], c["max_iterations"], precond)
        monkeypatch.setattr(gc, "dot", DOTS["numpy"])
        m, rp, ci, va, b = ed.onehot_compact(s)
        seq = gc.restate(m, rp, ci, va, b, np.zeros(m), 0.0, c["max_iterations"], c["restart"], precond,
                         spmv=gc.spmv_sequential)
        want = outs["numpy"]
        for order in DOTS:
            assert same_outcome(outs[order], want), (name, precond, order)
        assert np.array_equal(bits(seq[0]), bits(want[0][walk])) and tuple(seq[1:]) == tuple(want[1:]), (name, precond)
        x, it, restarts, conv, brk, rel = want
        assert brk == gc.NO_BREAKDOWN and np.all(x[np.setdiff1d(np.arange(n), walk)] == 0)
        nz = np.abs(x[x != 0])
        assert nz.min() > 2.0 ** -100 and nz.max() < 2.0 ** 100               # far from fp32's subnormals and its top
        if c["empty_column"] is None:
            assert (it, restarts, conv) == (c["max_iterations"], 2, False) and rel > 2.0 ** -100
        else:
            # six exact columns solve the closed 6 x 6 system: y is dyadic, x exact, r == 0 and 0 <= 0 converges
            k = c["empty_column"] + 1
            assert columns == k and (it, restarts, conv, rel) == (k, 0, True, 0.0)
            exact = np.zeros(k)
            for j in range(k):
                exact[j] = ((ed.ONEHOT_RHS if j == 0 else 0.0) - (s["beta"][walk[j - 1]] * exact[j - 1] if j else 0.0)) \
                    / s["d"][walk[j]]
            assert np.array_equal(x[walk[:k]], exact.astype(np.float32)) and np.count_nonzero(x) == k


@pytest.mark.parametrize("name", [nm for nm in ed.ONEHOT_NAMES if ed.ONEHOT_CASES[nm]["n"] < 5000])
def test_onehot_reference_on_the_walk_equals_the_restatement_on_the_whole_system(name):
    c, s = ed.onehot_case(name)
    for precond in (gc.NONE, gc.JACOBI):
        full = gc.restate(s["n"], s["rp"], s["ci"], s["va"], s["b"], np.zeros(s["n"]), 0.0, c["max_iterations"],
                          c["restart"], precond)
        assert same_outcome(ed.gmres_onehot_reference(s, c["restart"], c["max_iterations"], precond), full), \
            (name, precond)


def test_onehot_catalogue_reaches_the_paths_it_names():
    C = ed.ONEHOT_CASES
    chunk, blocks = ed.ONEHOT_CHUNK, ed.ONEHOT_ORTHO_BLOCKS
    # groups of eight: every restart of gmres_cases.RESTARTS, two full cycles and one column (closes with k = m, m, 1)
    assert {C["restart_%d" % m]["restart"] for m in gc.RESTARTS} == set(gc.RESTARTS)
    assert all(C["restart_%d" % m]["max_iterations"] == 2 * m + 1 for m in gc.RESTARTS)
    # vector tails: n mod 4 = 1, 2, 3; n-1, n-2, n-3, 0 and both sides of the first chunk edge
    tails = [C["tail_n3077"], C["tail_n3074"], C["restart_9"]]
    assert sorted(c["n"] % 4 for c in tails) == [1, 2, 3]
    for c in tails:
        assert {c["n"] - 1, c["n"] - 2, c["n"] - 3, 0, chunk - 1, chunk} <= set(c["visits"])
    # fold_columns: more than 64 and at most 256 workgroups, a ragged last chunk; first, 65th and last workgroup
    c = C["fold_second_trip"]
    groups = -(-c["n"] // chunk)
    assert ed.ONEHOT_FOLD_LANES * chunk < c["n"] <= blocks * chunk and c["n"] % chunk != 0
    assert {0, ed.ONEHOT_FOLD_LANES, groups - 1} <= set(c["chunks"]) and groups - 1 >= 2 * ed.ONEHOT_FOLD_LANES
    # basis kernels: more than 257 chunks; the chunk on either side of the wrap, and the last partial f32x4
    c = C["grid_second_trip"]
    assert c["n"] > (blocks + 1) * chunk and c["n"] % 4 != 0
    assert {blocks - 1, blocks, -(-c["n"] // chunk) - 1} <= set(c["chunks"])
    assert any(v >= c["n"] - c["n"] % 4 for v in c["visits"]) and any(v >= blocks * chunk for v in c["visits"])
    # the element-wise kernels (gmres_normalize) cap at kVecBlocks * 256 = 262 144 elements: the same case
    assert c["n"] > 1024 * 256
    # row loops at L = 1: 256 rows per workgroup, 2048 workgroups
    c = C["rows_second_trip"]
    edge = ed.ONEHOT_ROW_BLOCKS * 256
    assert c["n"] > edge and any(v >= edge for v in c["visits"]) and any(v < edge for v in c["visits"])
    # large cases keep the small basis
    assert all(c["restart"] <= 9 for c in C.values() if c["n"] > 5000)
    c = C["early_close"]
    assert 2 <= c["empty_column"] + 1 < c["restart"] - 1 and c["max_iterations"] > c["restart"]


# ------------------------------------------------------------------------------------------ GMRES, first step
@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_gmres_first_step_is_exact_per_lane_count(name):
    """exact_data.gmres_first_step asserts its derivation; here it runs for every lane count's system, and the
    prediction is the restatement's x after one step, bit for bit (the restatement rounds where the derivation says
    nothing is lost)."""
    L, n, rp, ci, va, b = ed.gmres_step_system(name)
    assert ed.lanes_for(int(rp[-1]), n) == L == int(name[1:].split("_")[0])
    assert np.count_nonzero(b) == 4 ** ed.GMRES_STEP_K <= n
    x1, y0 = ed.gmres_first_step(rp, ci, va, b, ed.GMRES_STEP_K)
    ref = gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, 1, 30, gc.NONE)
    assert np.array_equal(bits(ref[0]), bits(x1)) and ref[1:5] == (1, 0, False, gc.NO_BREAKDOWN)
    assert np.array_equal(x1 != 0, b != 0) and np.unique(np.abs(x1[x1 != 0])).size == 1


@pytest.mark.parametrize("W,R", ed.ENTRY_POINT_GEOMETRIES)
def test_gmres_first_tiled_step_system_is_exact(spmv, monkeypatch, W, R):
    n, rp, ci, va, b = ed.gmres_tiled_step_system(W)
    assert np.count_nonzero(b) == 4 ** ed.GMRES_TILED_STEP_K <= n == 20011
    x1, y0 = ed.gmres_first_step(rp, ci, va, b, ed.GMRES_TILED_STEP_K)
    ref = gc.restate(n, rp, ci, va, b, np.zeros(n), 0.0, 1, 2, gc.NONE)
    assert np.array_equal(bits(ref[0]), bits(x1)) and ref[1:5] == (1, 0, False, gc.NO_BREAKDOWN)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    assert spmv.tiled_shape(n, n, int(rp[-1])) == (True, W, R)
    assert int(np.diff(rp).max()) <= ed.default_long_row(-(-n // W))


# ------------------------------------------------------------------------------------------ two-eigenvalue systems
# cg.h's and bicgstab.h's algorithms in exact arithmetic: a vector is (int64 numerators, e) standing for num * 2^-e, a
# scalar a Fraction.  Every operation asserts what makes its fp32 / fp64 counterpart on the device exact.
from fractions import Fraction


def dy(num, e):
    """Normal form: the common trailing zero bits of the numerators moved into the exponent."""
    num = np.asarray(num, np.int64)
    low = int(np.bitwise_or.reduce(num)) if num.size else 0
    if low == 0:
        return np.zeros_like(num), 0
    shift = (low & -low).bit_length() - 1
    return num >> shift, e - shift


def dy_from(values):
    """A float array as a dyadic vector (every value a multiple of 2^-40 below 2^22: asserted)."""
    scaled = np.asarray(values, np.float64) * 2.0 ** 40
    assert np.array_equal(scaled, np.rint(scaled)) and np.abs(scaled).max(initial=0.0) < 2.0 ** 62
    return dy(scaled.astype(np.int64), 40)


def dy_float32(v):
    assert ed._fits_float32(v[0]), "an entry does not fit fp32's 24 bits"
    return np.ldexp(v[0].astype(np.float64), -v[1]).astype(np.float32)


def dy_frac(value, e):
    return Fraction(int(value), 1 << e) if e >= 0 else Fraction(int(value) << -e)


def dy_add(a, b):
    e = max(a[1], b[1])
    assert max(e - a[1], e - b[1]) < 40
    return dy((a[0] << (e - a[1])) + (b[0] << (e - b[1])), e)


def dyadic32(f):
    """A Fraction that fp32 holds: a power-of-two denominator, at most 24 significant bits."""
    den = f.denominator
    assert den & (den - 1) == 0, f
    num = abs(f.numerator)
    assert num != 0 and (num >> ((num & -num).bit_length() - 1)) < 1 << 24, f
    return f


def dy_scale(f, v):
    """f * v for a dyadic scalar."""
    den = f.denominator
    assert den & (den - 1) == 0
    assert abs(f.numerator) * int(np.abs(v[0]).max(initial=0)) < 1 << 62
    return dy(v[0] * f.numerator, v[1] + den.bit_length() - 1)


def dy_shift(v, k):
    """v[i] * 2^-k[i]: a multiplication by a power of two per row (dinv, or the diagonal factors' divisions)."""
    top = int(k.max())
    return dy(v[0] << (top - k), v[1] + top)


def dy_dot(a, b):
    """a.b as a Fraction; the sum of |terms| stays below 2^53 units: every partial sum is exact in fp64, any order."""
    bound = float(np.abs(a[0]).max(initial=0)) * float(np.abs(b[0]).max(initial=0)) * max(a[0].size, 1)
    assert bound < 2.0 ** 53, bound
    return dy_frac(int(np.dot(a[0], b[0])), a[1] + b[1])


def dy_spmv(matrix, x):
    """A x; per row the products are multiples of one quantum and their absolute sum is below 2^24 quanta, so every
    partial sum of the row, fused or not, in any order, is exact in fp32."""
    rp, ci, (num, e) = matrix
    prod = num * x[0][ci]
    assert float(np.abs(num).max()) * float(np.abs(x[0]).max(initial=0)) < 2.0 ** 62
    starts = rp[:-1].astype(np.int64)
    assert np.all(np.diff(rp) > 0)                                   # every row stores its diagonal
    any_bit = np.bitwise_or.reduceat(np.abs(prod), starts)
    quantum = any_bit & -any_bit
    assert np.all((np.add.reduceat(np.abs(prod), starts) >> 24) < quantum + (any_bit == 0))
    return dy(np.add.reduceat(prod, starts), e + x[1])


def two_eig_matrix(s):
    return s["rp"], s["ci"].astype(np.int64), dy_from(s["va"])


def dinv_shift(s):
    """k with dinv[i] = 2^-k[i], or None without a preconditioner: the stored diagonal is a power of two."""
    if not s["scaled"]:
        return None
    mant, expo = np.frexp(s["diag"])
    assert np.all(mant == 0.5)
    return (expo - 1).astype(np.int64)


def prove_cg(s, k):
    """cg.h from x0 = 0 in exact arithmetic; returns (x per step as float32, ||r|| / ||b|| per step, alphas, betas)."""
    A = two_eig_matrix(s)
    pre = (lambda v: v) if k is None else (lambda v: dy_shift(v, k))
    b = dy_from(s["b"])
    r = b
    z = pre(r)
    dy_float32(z)
    p, x = z, (np.zeros(s["n"], np.int64), 0)
    rz, bb = dy_dot(r, z), dy_dot(b, b)
    assert rz > 0
    xs, rels, alphas, betas = [], [], [], []
    for step in range(4):
        q = dy_spmv(A, p)
        dy_float32(q)
        pq = dy_dot(p, q)
        assert pq > 0
        alpha = dyadic32(rz / pq)
        x = dy_add(x, dy_scale(alpha, p))
        r = dy_add(r, dy_scale(-alpha, q))
        z = pre(r)
        xs.append(dy_float32(x)), dy_float32(r), dy_float32(z)
        rz_new, rr = dy_dot(r, z), dy_dot(r, r)
        alphas.append(alpha), rels.append(math.sqrt(rr / bb))
        if rr == 0:
            break
        assert rz_new > 0
        beta = dyadic32(rz_new / rz)
        betas.append(beta)
        p = dy_add(z, dy_scale(beta, p))
        dy_float32(p)
        rz = rz_new
    return xs, rels, alphas, betas


def prove_bicgstab(s, k):
    """bicgstab.h from x0 = 0 in exact arithmetic; returns (x per step as float32, residual per step, the scalars)."""
    A = two_eig_matrix(s)
    pre = (lambda v: v) if k is None else (lambda v: dy_shift(v, k))
    b = dy_from(s["b"])
    r = rhat = p = b
    x = (np.zeros(s["n"], np.int64), 0)
    rho, bb = dy_dot(r, r), dy_dot(b, b)
    xs, rels, scalars = [], [], []
    for step in range(4):
        ph = pre(p)
        v = dy_spmv(A, ph)
        dy_float32(ph), dy_float32(v)
        rv = dy_dot(rhat, v)
        assert rv != 0
        alpha = dyadic32(rho / rv)
        sv = dy_add(r, dy_scale(-alpha, v))
        sh = pre(sv)
        dy_float32(sv), dy_float32(sh)
        ss = dy_dot(sv, sv)
        half = dy_add(x, dy_scale(alpha, ph))                        # the inner multiply-add of the x update
        dy_float32(half)
        if ss == 0:
            xs.append(dy_float32(half)), rels.append(0.0), scalars.append((alpha,))
            break
        t = dy_spmv(A, sh)
        dy_float32(t)
        omega = dyadic32(dy_dot(t, sv) / dy_dot(t, t))
        x = dy_add(half, dy_scale(omega, sh))
        r = dy_add(sv, dy_scale(-omega, t))
        xs.append(dy_float32(x)), dy_float32(r)
        rr, rho_new = dy_dot(r, r), dy_dot(rhat, r)
        rels.append(math.sqrt(rr / bb))
        assert rr != 0 and rho_new != 0
        dyadic32(rho_new / rho), dyadic32(alpha / omega)             # both fp64 quotients of beta are exact
        beta = dyadic32((rho_new / rho) * (alpha / omega))
        scalars.append((alpha, omega, beta))
        inner = dy_add(p, dy_scale(-omega, v))
        dy_float32(inner)
        p = dy_add(r, dy_scale(beta, inner))
        dy_float32(p)
        rho = rho_new
    return xs, rels, scalars


def assert_two_eig_structure(s):
    """Sets, symmetry, dominance, raggedness, the lane count and what the grid-stride trips see, on the UNSCALED
    system (the scaled one is T A T entry by entry: asserted by the caller)."""
    assert not s["scaled"]
    n, L, rp, ci = s["n"], s["L"], s["rp"], s["ci"]
    rows = np.repeat(np.arange(n), np.diff(rp))
    vals = s["va"].astype(np.float64)
    assert ed.lanes_for(int(rp[-1]), n) == L
    assert np.unique(np.diff(rp)).size >= 3                                       # ragged
    assert np.array_equal(s["sets"][rows], s["sets"][ci]) and np.count_nonzero(s["sets"] == 0) <= 3
    assert np.unique(rows.astype(np.int64) * n + ci).size == ci.size              # no (row, column) twice
    on = rows == ci
    assert np.count_nonzero(on) == n and np.array_equal(vals[on], s["diag"][rows[on]].astype(np.float64))
    key = rows.astype(np.int64) * n + ci
    forward, backward = np.argsort(key), np.argsort(ci.astype(np.int64) * n + rows)
    mirrored = np.array_equal(key[forward], (ci.astype(np.int64) * n + rows)[backward])
    if s["symmetric"]:
        assert mirrored and np.array_equal(vals[forward], vals[backward])
        off = np.bincount(rows[~on], weights=np.abs(vals[~on]), minlength=n)
        assert np.all(off < ed.TWO_EIG_D)                                         # strictly diagonally dominant: SPD
    else:
        assert not mirrored                                                       # not even the pattern is symmetric
    for trip in {ed.VEC_TRIP, ed.row_trip(L)}:
        if n > trip:
            trips = -(-n // trip)
            for t in range(trips):                                                # (a last trip of ONE row holds one set)
                want = {1, 2} if min(n, (t + 1) * trip) - t * trip >= 2 else {1}
                assert set(np.unique(s["sets"][t * trip:(t + 1) * trip])) >= want, (trip, t)
            assert np.count_nonzero((rows // trip != ci // trip) & ~on) > 0
            other = np.unique(rows[(rows // trip) != (ci // trip)] // trip)
            assert other.size == trips                                            # rows of every trip read another trip


TWO_EIG_CASES = [(solver, n, L) for solver in ("cg", "bicgstab")
                 for n, L in [(n, 1) for n in ed.TRIP_SIZES] + [(ed.LANE_SIZES[L], L) for L in ed.LANES[1:]]]


@pytest.mark.parametrize("solver,n,L", TWO_EIG_CASES)
def test_two_eig_system_is_exact_to_its_last_step(solver, n, L):
    """Every system tests/test_gpu_solver_trips.py runs, unscaled (NONE) and scaled (JACOBI, IC, LU): the documented
    algorithm in integers ends at step 2 with r == 0, every stored vector fits fp32, every row sum and dot product is
    exact in any order, alpha / beta / omega are dyadic, and x1, x2 and the one-step residual are the builder's."""
    for scaled in (False, True):
        s = ed.two_eig_system(solver, n, L, scaled)
        if not scaled:
            assert_two_eig_structure(s)
            plain = s
        else:                                                                      # A' = T A T, b' = T b, same pattern
            rows = np.repeat(np.arange(n), np.diff(s["rp"]))
            assert np.array_equal(s["ci"], plain["ci"]) and np.unique(s["e"]).size >= 2
            assert np.array_equal(s["va"], np.ldexp(plain["va"], s["e"][rows] + s["e"][s["ci"]]))
            assert np.array_equal(s["b"], np.ldexp(plain["b"], s["e"]))
            assert np.array_equal(s["diag"], np.ldexp(np.float32(ed.TWO_EIG_D), 2 * s["e"]))
        k = dinv_shift(s)
        if solver == "cg":
            xs, rels, alphas, betas = prove_cg(s, k)
            top = Fraction(2) if scaled else Fraction(2, ed.TWO_EIG_D)
            assert alphas == [top, top] and betas == [Fraction(1, 2)]
        else:
            xs, rels, scalars = prove_bicgstab(s, k)
            unit = Fraction(1) if scaled else Fraction(1, ed.TWO_EIG_D)
            assert scalars == [(8 * unit, -2 * unit, Fraction(3)), (-2 * unit,)]
        assert len(xs) == 2 and rels[1] == 0.0 and rels[0] > 1e-3                  # no early stop at tolerance 1e-6
        assert np.array_equal(bits(xs[0]), bits(s["x1"])) and np.array_equal(bits(xs[1]), bits(s["x2"]))
        got, want = np.float32(rels[0]), s["rel1"]
        assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1        # two roundings apart at most
        if scaled:                                                                 # the diagonal factors of IC and LU
            root = np.sqrt(s["diag"])
            assert np.array_equal(root * root, s["diag"]) and np.all(np.frexp(root)[0] == 0.5)


@pytest.mark.parametrize("solver", ["cg", "bicgstab"])
@pytest.mark.parametrize("n", [257, 1201])
def test_two_eig_prediction_is_the_restatement_bit_for_bit(solver, n):
    """test_gpu_cg.restate / test_gpu_bicgstab.restate in plain floating point give the predicted x, counts and flags:
    the prediction is tied to the documented algorithm, not to a second derivation."""
    restate = importlib.import_module("test_gpu_cg" if solver == "cg" else "test_gpu_bicgstab").restate
    for scaled in (False, True):
        s = ed.two_eig_system(solver, n, 1, scaled)
        args = (n, s["rp"], s["ci"], s["va"], s["b"], np.zeros(n, np.float32))
        x, it, conv, brk, rel = restate(*args, 1e-6, 50, int(scaled))
        assert (it, bool(conv), int(brk), float(rel)) == (2, True, 0, 0.0)
        assert np.array_equal(bits(x), bits(s["x2"]))
        x, it, conv, brk, rel = restate(*args, 0.0, 1, int(scaled))
        assert (it, bool(conv), int(brk)) == (1, False, 0) and np.float32(rel) == s["rel1"]
        assert np.array_equal(bits(x), bits(s["x1"]))


@pytest.mark.parametrize("L", ed.LANES[1:])
def test_init_solution_is_exact_at_the_lane_sweep_sizes(L):
    for solver in ("cg", "bicgstab"):
        s = ed.two_eig_system(solver, ed.LANE_SIZES[L], L, scaled=False)
        x_star, b = ed.init_solution(s)                                            # check_exact inside
        assert s["n"] > ed.row_trip(L) and np.count_nonzero(b) > 0.9 * s["n"]


def test_trip_sizes_reach_the_edges_they_name():
    V, sizes = ed.VEC_TRIP, ed.TRIP_SIZES
    assert V == 262144 and ed.row_trip(1) == 524288
    assert sizes[:2] == [257, 1201] and sizes[2:] == [V, V + 1, V + 257, 2 * V + 3, ed.row_trip(1) + 257]
    assert sum(n > 2 * V for n in sizes) == 2                                      # a third element-wise trip twice
    for L, n in ed.LANE_SIZES.items():
        assert n == ed.row_trip(L) + 256 // L + 1                                  # one full workgroup and one row more


@pytest.mark.parametrize("L", ed.SPTRSV_TRIP_LANES)
def test_two_level_triangle_has_two_wide_levels_and_an_integer_solution(spmv, L):
    for uplo in (0, 1):
        for unit in (0, 1):
            c = ed.two_level_triangle(L, uplo, unit)
            n, rp, ci, half = c["n"], c["rp"], c["ci"], c["half"]
            assert n == 2 * ed.row_trip(L) + 2 * (256 // L) + 2 and half > ed.row_trip(L)
            _, level_ptr, order, levels, _ = spmv.sptrsv_levels(n, rp, ci, uplo)
            assert levels == 2 and list(np.diff(level_ptr)) == [half, half]
            rows = np.repeat(np.arange(n), np.diff(rp))
            inside = (ci < rows) if uplo == 0 else (ci > rows)
            assert np.all((ci == rows) | inside)                                   # nothing in the other triangle
            on = ci == rows
            d = np.ones(n) if unit else c["va"][on][np.argsort(rows[on])].astype(np.float64)
            assert np.all(np.frexp(d)[0] == 0.5)                                   # powers of two
            eff = np.where(on & bool(unit), 1.0, c["va"].astype(np.float64))
            x = c["x"].astype(np.float64)
            assert np.array_equal(np.bincount(rows, weights=eff * x[ci], minlength=n), c["b"].astype(np.float64))
            assert np.bincount(rows, weights=np.abs(eff * x[ci]), minlength=n).max() < ed.EXACT_LIMIT
            # position k of the second level lies in trip k // R_L; its columns lie in both trips of the first level
            second = np.asarray(order)[half:]
            place = np.empty(n, np.int64)
            place[np.asarray(order)[:half]] = np.arange(half)
            trip_of_row = np.empty(n, np.int64)
            trip_of_row[second] = np.arange(half) // ed.row_trip(L)
            dep = inside
            assert np.count_nonzero(trip_of_row[rows[dep]] != place[ci[dep]] // ed.row_trip(L)) > 0
            assert np.unique(np.diff(rp)).size >= 3


# ------------------------------------------------------------------------------------------ one-hot Lanczos systems
ec = importlib.import_module("eigs_cases")
SPMVS = {"round once": gc.spmv_round_once, "sequential": gc.spmv_sequential}
WHICH = (ec.LARGEST, ec.SMALLEST)


def lanczos_variants(monkeypatch, run):
    """{(dot order, SpMV order): run(spmv)} over three dot-product orders x two SpMV orders of eigs_cases.restate"""
    outs = {}
    for order, dot in DOTS.items():
        monkeypatch.setattr(gc, "dot", dot)
        for name, spmv in SPMVS.items():
            outs[(order, name)] = run(spmv)
    monkeypatch.setattr(gc, "dot", DOTS["numpy"])
    return outs


def same_pairs(got, want, residuals=False):
    """every field of restate's dict but the residuals (unless asked for): values and vectors on the bits"""
    fields = ("found", "converged", "iterations", "restarts", "breakdown")
    nan_equal = lambda a, b: np.array_equal(bits(a), bits(b)) or (np.all(np.isnan(a) == np.isnan(b)) and
                                                                  np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)])))
    same = (all(got[f] == want[f] for f in fields) and nan_equal(got["values"], want["values"])
            and np.array_equal(bits(got["vectors"]), bits(want["vectors"])))
    if residuals:
        same = same and nan_equal(got["residuals"], want["residuals"]) and \
            bits(np.float32(got["max_residual"])) == bits(np.float32(want["max_residual"]))
    return same


def lanczos_first_cycle(system, columns):
    """The first cycle's Lanczos steps on the walk positions, spelled out, with the module comment's claims asserted per
    column and per dot-product order: h1 is d_(q_j) at i = j, |beta_(q_j)| at i = j - 1 and 0.0 elsewhere, the updated w
    is one-hot at q_j+1 with sign_j beta_(q_j+1), h2 is all 0.0, sqrt(w.w) == |beta| with a power-of-two inverse and
    v_j+1 == sign_j+1 e_(q_j+1)."""
    m, rp, ci, va, v0 = ed.lanczos_onehot_compact(system)
    walk, d, beta, sign = system["walk"], system["d"], system["beta"], system["sign"]
    assert np.sqrt(gc.dot(v0, v0)) == ed.LANCZOS_START
    V = [(v0 * np.float32(1.0 / ed.LANCZOS_START)).astype(np.float32)]
    assert V[0][0] == 1.0 == sign[0] and np.count_nonzero(V[0]) == 1
    for j in range(columns):
        ws = [spmv(rp, ci, va, V[j]) for spmv in SPMVS.values()]
        assert np.array_equal(ws[0], ws[1]) and np.count_nonzero(ws[0]) <= 3       # equal values: a zero's sign may differ
        w = ws[0]
        for dot in DOTS.values():
            h1 = [np.float32(dot(v, w)) for v in V]
            assert h1[j] == d[walk[j]] and all(h == 0.0 for h in h1[:max(j - 1, 0)])
            assert j == 0 or h1[j - 1] == abs(beta[walk[j]])
        for hi, v in zip(h1, V):
            w = gc.fma(-hi, v, w)
        if system["cut"] == j:
            assert np.count_nonzero(w) == 0                      # the invariant space: beta == 0
            return j + 1
        assert np.count_nonzero(w) == 1 and w[j + 1] == sign[j] * beta[walk[j + 1]]
        for dot in DOTS.values():
            assert all(np.float32(dot(v, w)) == 0.0 for v in V)     # h2
            hn = np.sqrt(dot(w, w))
            assert hn == abs(beta[walk[j + 1]]) and np.frexp(np.float32(1.0 / hn))[0] == 0.5
        V.append((w * np.float32(1.0 / hn)).astype(np.float32))
        assert np.count_nonzero(V[-1]) == 1 and V[-1][j + 1] == sign[j + 1] and abs(sign[j + 1]) == 1.0
    return columns


@pytest.mark.parametrize("name", ed.LANCZOS_NAMES)
def test_lanczos_case_is_what_it_claims(monkeypatch, name):
    """No revisit, the required positions, powers of two, symmetry, L = 1, the first cycle's exactness claims column by
    column, and per run and end of the spectrum the same bits in values and vectors from three dot-product orders x two
    SpMV orders, equal to the prediction from the walk's tridiagonal matrix alone."""
    c, s = ed.lanczos_case(name)
    n, walk, rp, ci, va = s["n"], s["walk"], s["rp"], s["ci"], s["va"]
    assert walk.size == c["steps"] + 1 == np.unique(walk).size and walk[0] == c["p"]
    columns_wanted = max(min(cc, mm) for _, mm, cc in c["runs"])
    reach = walk[:columns_wanted + 1]                                # the columns of the longest run and its next vector
    assert set(c["visits"]) <= set(reach.tolist()) and set(c["chunks"]) <= set((reach // ed.ONEHOT_CHUNK).tolist())
    assert n % 64 != 0 and n % 4 != 0
    nnz = int(rp[-1])
    assert nnz == 3 * n - 2 * (1 + (c["cut"] is not None)) and ed.lanes_for(nnz, n) == 1 and int(np.diff(rp).max()) == 3
    assert np.all(np.frexp(np.abs(va))[0] == 0.5) and np.abs(np.frexp(va)[1] - 1).max() <= 1
    assert np.count_nonzero(s["v0"]) == 1 and s["v0"][c["p"]] == ed.LANCZOS_START
    rows = np.repeat(np.arange(n), np.diff(rp))
    key = rows.astype(np.int64) * n + ci
    assert np.unique(key).size == nnz                                 # distinct columns inside a row
    mirror = np.sort(ci.astype(np.int64) * n + rows)
    order = np.argsort(key)
    assert np.array_equal(key[order], mirror)                         # the pattern is symmetric ...
    assert np.array_equal(va[order], va[np.argsort(ci.astype(np.int64) * n + rows)])      # ... and so are the values
    off = ci != rows
    assert np.all(((ci[off] + c["s"]) % n == rows[off]) | ((ci[off] - c["s"]) % n == rows[off]))
    assert np.array_equal(np.sort(ci[~off]), np.arange(n))
    back = (c["p"] - c["s"]) % n
    assert not np.any((rows == c["p"]) & (ci == back)) and not np.any((rows == back) & (ci == c["p"]))
    if c["nan_step"] is not None:
        bad = ed.lanczos_nan_values(c, s)
        at = np.flatnonzero(np.isnan(bad))
        assert at.size == 1 and rows[at[0]] == ci[at[0]] == walk[c["nan_step"]] >= ed.ONEHOT_ROW_BLOCKS * 256
        k, m, cap = c["runs"][0]
        out = ed.lanczos_onehot_reference(dict(s, va=bad), k, ec.LARGEST, m, cap)
        assert (out["breakdown"], out["iterations"], out["found"]) == (ec.NOT_FINITE, 0, 0)
        assert np.all(np.isnan(out["values"])) and not out["vectors"].any()
        return
    assert lanczos_first_cycle(s, columns_wanted) == (columns_wanted if c["cut"] is None else c["cut"] + 1)
    for k, m, cap in c["runs"]:
        assert 1 <= k < m <= ec.MAX_ORDER and k <= 32                 # what eigs.h admits
        cols = min(cap, m) if c["cut"] is None else c["cut"] + 1
        assert cap <= m or c["cut"] is not None                       # no restart
        for which in WHICH:
            outs = lanczos_variants(monkeypatch, lambda spmv: ed.lanczos_onehot_reference(s, k, which, m, cap, spmv))
            want = outs[("numpy", "round once")]
            for variant, out in outs.items():
                assert same_pairs(out, want), (name, k, m, cap, which, variant)
            found = min(k, cols)
            assert (want["iterations"], want["restarts"], want["found"], want["converged"]) == (cols, 0, found, 0)
            assert want["breakdown"] == (ec.INVARIANT_SUBSPACE if c["cut"] is not None and found < k else ec.NO_BREAKDOWN)
            values, vectors = ed.lanczos_onehot_prediction(s, k, which, cols)
            assert np.array_equal(bits(values[:found]), bits(want["values"][:found])), (name, k, m, cap, which)
            assert np.all(np.isnan(values[found:])) and np.all(np.isnan(want["values"][found:]))
            assert np.array_equal(bits(vectors), bits(want["vectors"])), (name, k, m, cap, which)
            assert not vectors[:, np.setdiff1d(np.arange(n), walk[:cols])].any() and not vectors[found:].any()
            assert np.all(want["residuals"][:found] > 0)              # tolerance 0 converges nothing


@pytest.mark.parametrize("name", [nm for nm in ed.LANCZOS_NAMES if ed.LANCZOS_CASES[nm]["n"] < 5000])
def test_lanczos_reference_on_the_walk_equals_the_restatement_on_the_whole_system(name):
    c, s = ed.lanczos_case(name)
    for k, m, cap in c["runs"]:
        for which in WHICH:
            full = ec.restate(s["n"], s["rp"], s["ci"], s["va"], k, which, m, tol=0.0, max_iter=cap, v0=s["v0"])
            assert same_pairs(ed.lanczos_onehot_reference(s, k, which, m, cap), full, residuals=True), (name, k, m, which)


def test_lanczos_catalogue_reaches_the_paths_it_names():
    """Every edge is derived from the constants of csrc/basis_ops.h and csrc/device_common.h as restated in exact_data:
    a changed kChunk, kOrthoBlocks, kVecBlocks or kMaxResidentBlocks fails here, not silently on the GPU."""
    C = ed.LANCZOS_CASES
    chunk, blocks, fold = ed.ONEHOT_CHUNK, ed.ONEHOT_ORTHO_BLOCKS, ed.ONEHOT_FOLD_LANES
    assert chunk == 4 * 256 and ed.VEC_TRIP == 1024 * 256 and ed.ROW_TRIP_THREADS == ed.ONEHOT_ROW_BLOCKS * 256
    columns = lambda c: max(min(cc, mm) for _, mm, cc in c["runs"])
    # the basis edges: one column, a group of eight less one, full, plus one, two groups, plus one, the cap and one less;
    # per edge k = 1, min(c, 32), min(c + 2, 32), run at the basis c where eigs.h admits it (k < m)
    assert ed.LANCZOS_BASIS_EDGES == (1, 2, 7, 8, 9, 16, 17, 63, 64)
    for c in ed.LANCZOS_BASIS_EDGES:
        runs = C["basis_%d" % c]["runs"]
        assert {k for k, _, _ in runs} == {1, min(c, 32), min(c + 2, 32)} and all(cc == c for _, _, cc in runs)
        assert all((m == c) if k < c else (m == k + 1) for k, m, _ in runs)
        assert c < 2 or any(m == c for _, m, _ in runs)               # a close on j + 1 == m at every edge but c = 1
        assert C["basis_%d" % c]["n"] == 4103
    assert any(k > cc for k, _, cc in C["basis_1"]["runs"]) and any(k > cc for k, _, cc in C["basis_17"]["runs"])
    # a close on the budget, one column before the basis is full
    assert any(cc == m - 1 and k < cc for k, m, cc in C["budget_before_basis"]["runs"])
    # vector tails: n mod 4 = 1, 2, 3; n-1, n-2, n-3, 0 and both sides of the first chunk edge, inside the columns
    tails = [C["tail_n3077"], C["tail_n3074"], C["basis_16"]]
    assert sorted(c["n"] % 4 for c in tails) == [1, 2, 3]
    for c in tails:
        assert {c["n"] - 1, c["n"] - 2, c["n"] - 3, 0, chunk - 1, chunk} <= set(c["visits"])
        _, s = ed.lanczos_case(c["name"])
        assert set(c["visits"]) <= set(s["walk"][:columns(c)].tolist())
    # fold_columns: more than 64 and at most 256 workgroups, a ragged last chunk; first, 65th and last workgroup
    c = C["fold_second_trip"]
    groups = -(-c["n"] // chunk)
    assert fold * chunk < c["n"] <= blocks * chunk and c["n"] % chunk != 0
    assert {0, fold, groups - 1} <= set(c["chunks"]) and groups - 1 >= 2 * fold
    # the basis kernels' grid stride (ogrid = 256), the element-wise kernels (vgrid = 1024 workgroups of 256) and
    # fold_partials with count = vgrid > 256: more than 257 chunks, both sides of the wrap, the last partial f32x4
    c = C["grid_second_trip"]
    assert c["n"] > (blocks + 1) * chunk and c["n"] % 4 != 0 and c["n"] > ed.VEC_TRIP
    assert min(-(-c["n"] // 256), 1024) > 256                         # vgrid: fold_partials' count in eigs_start / eigs_verdict
    assert {blocks - 1, blocks, -(-c["n"] // chunk) - 1} <= set(c["chunks"])
    assert any(v >= c["n"] - c["n"] % 4 for v in c["visits"]) and any(v >= ed.VEC_TRIP for v in c["visits"])
    assert any(v < ed.VEC_TRIP for v in c["visits"])
    # eigs_spmv<1>, eigs_rotate<true> (2048 workgroups of 256 elements) and eigs_fill_failed: both sides of 524 288
    edge = ed.row_trip(1)
    for c in (C["rows_second_trip"], C["nan_on_the_walk"]):
        assert c["n"] > edge and any(v >= edge for v in c["visits"]) and any(v < edge for v in c["visits"])
    assert any(k > cc for k, _, cc in C["rows_second_trip"]["runs"])          # zero rows written past the edge
    # large cases keep the small basis
    assert all(m <= 9 for c in C.values() if c["n"] > 5000 for _, m, _ in c["runs"])
    c = C["invariant_mid_cycle"]
    assert all(2 <= c["cut"] + 1 < m - 1 and cap > m for _, m, cap in c["runs"])
    assert {k for k, _, _ in c["runs"]} >= {c["cut"] + 1, c["cut"] + 3}       # k == the invariant space's order, and beyond
    # thick restarts: elements past both edges, and the one small case
    R = ed.LANCZOS_RESTART_CASES
    assert {(k, m) for g, k, m in R if g == "grid_second_trip"} == {(2, 8), (2, 9)} == \
        {(k, m) for g, k, m in R if g == "rows_second_trip"}
    assert ("restart_9", 4, 20) in R and all(m < 64 for _, _, m in R)
    for g, k, m in R:
        s, cap = ed.lanczos_restart_case(g, k, m)
        assert cap == 2 * m + 1 and s["walk"].size == cap + 2
        if g != "restart_9":
            limit = ed.VEC_TRIP if g == "grid_second_trip" else edge
            assert np.any(s["walk"][:m] >= limit) and np.any(s["walk"] < limit)


# ------------------------------------------------------------------------------------------ Lanczos, first step
def assert_first_step(monkeypatch, n, rp, ci, va, v0, step, name):
    """the six restatement variants agree on the bits, residuals included, and equal lanczos_first_step's prediction"""
    k = ed.LANCZOS_STEP_VALUES
    outs = lanczos_variants(monkeypatch, lambda spmv: ec.restate(n, rp, ci, va, k, ec.LARGEST, k + 1, tol=0.0, max_iter=1,
                                                                 v0=v0, spmv=spmv))
    want = outs[("numpy", "round once")]
    for variant, out in outs.items():
        assert same_pairs(out, want, residuals=True), (name, variant)
    assert (want["iterations"], want["restarts"], want["found"]) == (1, 0, 1)
    assert bits(want["values"][0]) == bits(step["value"]) and np.all(np.isnan(want["values"][1:]))
    assert np.array_equal(bits(want["vectors"][0]), bits(step["vector"])) and not want["vectors"][1:].any()
    assert bits(want["residuals"][0]) == bits(step["residual"]) and np.all(np.isnan(want["residuals"][1:]))
    assert bits(np.float32(want["max_residual"])) == bits(step["residual"])
    assert want["converged"] == step["converged"]
    assert want["breakdown"] == (ec.INVARIANT_SUBSPACE if step["invariant"] else ec.NO_BREAKDOWN)


@pytest.mark.parametrize("name", ed.SOLVER_NAMES)
def test_lanczos_first_step_is_exact_per_lane_count(monkeypatch, name):
    """exact_data.lanczos_first_step asserts its derivation; here it runs for every lane count's symmetric system, and
    the prediction is the restatement's after one step, bit for bit in values, vectors and residuals, in six orders."""
    L, n, rp, ci, va, v0, step = ed.lanczos_step_system(name)
    assert ed.lanes_for(int(rp[-1]), n) == L == int(name[1:].split("_")[0])
    assert np.count_nonzero(v0) == 4 ** ed.LANCZOS_STEP_K <= n
    assert_first_step(monkeypatch, n, rp, ci, va, v0, step, name)
    if name == "L1_low":                      # the diagonal and one pair: A v0 == v0
        assert (step["invariant"], step["converged"], step["value"], step["residual"]) == (True, 1, 1.0, 0.0)
    else:
        assert not step["invariant"] and step["converged"] == 0 and step["residual"] > 0


@pytest.mark.parametrize("L", ed.LANCZOS_TRIP_LANES)
def test_lanczos_trip_system_puts_the_step_on_both_sides_of_the_row_loop(monkeypatch, L):
    n, rp, ci, va, v0, step = ed.lanczos_trip_system(L)
    edge = ed.row_trip(L)
    assert n == ed.LANE_SIZES[L] > edge and ed.lanes_for(int(rp[-1]), n) == L
    assert np.count_nonzero(v0) == 4 ** ed.LANCZOS_STEP_K
    for mask in (v0 != 0, step["ab"] != 0, step["num"] != 0):
        assert mask[:edge].any() and mask[edge:].any()
    assert_first_step(monkeypatch, n, rp, ci, va, v0, step, L)


def test_lanczos_first_tiled_step_system_is_exact(spmv, monkeypatch):
    W, R = ed.ENTRY_POINT_GEOMETRIES[0]
    n, rp, ci, va, v0, step = ed.lanczos_tiled_step_system(W)
    assert np.count_nonzero(v0) == 4 ** ed.LANCZOS_TILED_STEP_K <= n == 20011
    assert_first_step(monkeypatch, n, rp, ci, va, v0, step, "tiled")
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    assert spmv.tiled_shape(n, n, int(rp[-1])) == (True, W, R)
    assert int(np.diff(rp).max()) <= ed.default_long_row(-(-n // W))


# ------------------------------------------------------------------------------------------ Lanczos, thick restarts
@pytest.mark.parametrize("geometry,k,m", ed.LANCZOS_RESTART_CASES)
def test_lanczos_restart_case_leaves_the_device_room(monkeypatch, geometry, k, m):
    """The condition for a thick-restart case to be in the catalogue: six restatement orders agree in iterations,
    restarts and found, and in the values within VALUE_BOUND / 2 of max |lambda|: the device's seventh order has the same
    room again.  Prints the spread it measures."""
    s, cap = ed.lanczos_restart_case(geometry, k, m)
    assert ed.lanes_for(int(s["rp"][-1]), s["n"]) == 1
    lmax = ed.lanczos_lambda_max(s)
    for which in WHICH:
        outs = lanczos_variants(monkeypatch, lambda spmv: ed.lanczos_onehot_reference(s, k, which, m, cap, spmv))
        want = outs[("numpy", "round once")]
        assert want["iterations"] == cap and want["restarts"] >= 1 and want["found"] == k
        assert want["breakdown"] == ec.NO_BREAKDOWN and want["converged"] == 0
        spread = 0.0
        for variant, out in outs.items():
            assert (out["iterations"], out["restarts"], out["found"]) == (cap, want["restarts"], k), variant
            spread = max(spread, float(np.max(np.abs(out["values"].astype(np.float64) - want["values"]))) / lmax)
        print(geometry, k, m, which, "restarts", want["restarts"], "spread %.2e x lambda_max" % spread)
        assert 2 * spread <= ec.VALUE_BOUND / 2                       # any two variants lie within VALUE_BOUND / 2
