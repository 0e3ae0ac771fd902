"""Sharded (multi-GPU) PageRank held to the BITS of the integer prover, on one device.

The graph is exact_data.SHARDED_CASE: n = 2^16, damping 0.5, out-degrees 2 and 4, two hub rows, 4096 dangling nodes
drawn from the nodes nobody links to.  exact_data.exact_steps proves (tests/test_exact_data.py, no GPU) that three
steps of r_new = d * (A r) + d * s / n + (1 - d) / n are exact in float32, dangling mass included: every summation
order gives the same bits, so EVERY way of cutting the rows, numbering the vector and exchanging the slices must give
the bits of exact_data.dyadic_trajectory after EVERY step on EVERY rank.  The dangling mass of steps 2 and 3 is the
one the device accumulated (block partials -> pr_reduce -> tails / sums -> pr_commit*), crossing ranks on the way.
No tolerance anywhere except the residual (4 float32 ulps: the kernels round each squared difference to float32).

Part 1 drives the shard engine (csrc/pagerank.hip behind HipEngine, Layout of pagerank_dist.py) with the host playing
the exchange (tests/shard_sim.py); part 2 drives the native one-process loop (csrc/pagerank_multi.cpp, its own
partition and renumbering) through pagerank() with SPMV_NUM_GPUS=P and SPMV_MULTI_GPU=share_devices.  Every case
prints the configuration it ran (world, bounds, chunks, piece, block, plan shapes) and asserts the engine it claims."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import shard_sim

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
pagerank_tests = importlib.import_module("test_gpu_pagerank")
assert_bits = sweep.assert_bits
W, R = ed.SHARD_W, ed.SHARD_R
DAMPING = ed.DYADIC_DAMPING


def graph():
    """(n, rp, ci, va, steps, [(ranks, residual) after step 1..steps], dangling nodes, hub row)"""
    n, rp, ci, va, steps, _, _ = ed.dyadic_case(ed.SHARDED_CASE)
    assert steps >= 3
    trajectory = ed.dyadic_trajectory(rp, ci, va, n, DAMPING, steps)
    dangling = np.flatnonzero(np.bincount(ci, minlength=n) == 0)
    return n, rp, ci, va, steps, trajectory, dangling, ed.DYADIC_SOURCES[ed.SHARDED_CASE](n)[0][0]


@pytest.fixture
def world_of(gpu, monkeypatch):
    """make(tiled, world, ...) -> shard_sim.Sim over the graph, SPMV_DEBUG set so that the shards run the tiled
    engine at (W, R) or the direct kernel; the engines asserted, the configuration printed; closed afterwards."""
    torch = pytest.importorskip("torch")
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    n, rp, ci, va = graph()[:4]
    made = []

    def make(tiled, world, what="", **layout):
        if tiled:
            monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
            monkeypatch.setenv("SPMV_TILED_FOLD", "1")
        else:
            monkeypatch.delenv("SPMV_DEBUG", raising=False)
        sim = shard_sim.Sim(gpu, prd, torch, rp, ci, va, n, world, **layout)
        made.append(sim)
        sim.assert_engines(tiled, W, R)
        print(what, "tiled" if tiled else "direct", sim.describe())
        return sim

    yield make
    for sim in made:
        sim.close()


def run_and_check(sim, what, mode="gather", **step):
    """Every exact step, every rank: the prover's bits, identical vectors and states, residual, padding."""
    _, _, _, _, steps, trajectory, _, _ = graph()
    for k in range(steps):
        sim.step(k, DAMPING, 0.0, mode=mode, **step)
        sim.check(k, trajectory[k][0], trajectory[k][1], assert_bits, what)


def spread(bounds, min_rows=100):
    """Per-rank dangling counts; every rank of more than min_rows rows owns some, and no two own the same number:
    a commit that takes one rank's partial mass for every rank cannot give the prover's s."""
    counts = ed.dangling_per_rank(bounds, graph()[6])
    big = np.diff(np.asarray(bounds)) > min_rows
    assert (counts[big] > 0).all() and np.unique(counts[big]).size == int(big.sum()), counts
    return counts


# ------------------------------------------------------------------------------------------ world sizes
WORLD_CASES = [(1, "rows")] + [(w, cut) for w in ed.SHARD_WORLDS[1:] for cut in ("rows", "nnz")]


@pytest.mark.parametrize("tiled", [False, True], ids=["direct", "tiled"])
@pytest.mark.parametrize("world,cut", WORLD_CASES)
def test_world_sizes_and_both_cuts(world_of, world, cut, tiled):
    """World 1 (no exchange: step_and_commit), 2, 3, 5, 8; rows cut equally (odd shard lengths rounded up to even,
    n not reached by world * shard_len at 3 and 5) and for equal nnz; pr_step_kernel and the tiled engine."""
    n, rp = graph()[:2]
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    bounds = None if cut == "rows" else prd.Layout.equal_nnz_bounds(rp, world)
    sim = world_of(tiled, world, ("world", world, cut), bounds=bounds)
    counts = spread(sim.lays[0].bounds)
    assert world == 1 or (counts.size == world and counts.min() > 0)
    run_and_check(sim, ("world", world, cut, tiled), mode="local" if world == 1 else "gather")


# ------------------------------------------------------------------------------------------ cut edges
@pytest.mark.parametrize("tiled", [False, True], ids=["direct", "tiled"])
@pytest.mark.parametrize("name", list(ed.shard_cut_edges(1 << 16, 0)))
def test_cut_edges(world_of, name, tiled):
    """Explicit bounds: a shard without rows (first, middle, last), a shard of one empty row (nnz == 0, column
    pointer 0), a hub row alone in its shard, cuts right before and right after a hub, an odd longest shard."""
    n, _, _, _, _, _, _, hub = graph()
    bounds = ed.shard_cut_edges(n, hub)[name]
    sim = world_of(tiled, len(bounds) - 1, ("cut", name), bounds=bounds)
    spread(bounds)
    run_and_check(sim, ("cut", name, tiled))


# ------------------------------------------------------------------------------------------ chunk-major layout
@pytest.mark.parametrize("align", ed.SHARD_ALIGNS)
@pytest.mark.parametrize("chunks", ed.SHARD_CHUNKS)
def test_chunk_major_layout_with_head_start(world_of, chunks, align):
    """Layout(chunks=C): RowMap.at on the device, remap_columns, the tail at the end of the LAST piece, pieces of a
    short shard without rows; the tiled engine with a head start per block, foreign pieces poisoned with NaN wherever
    the engine must not look.  align = 1000: block boundaries fall inside strips of 4096 columns, so pr_expand has
    to round cols_ready / strip_cols DOWN (a strip expanded early would multiply NaN)."""
    n = graph()[0]
    world, bounds = ed.chunk_world(n, chunks)
    sim = world_of(True, world, ("chunks", chunks, "align", align), bounds=bounds, chunks=chunks, align=align)
    lay = sim.lays[0]
    assert lay.chunks == chunks and lay.piece % align == 0
    inside = [c for c in range(1, chunks) if (c * lay.block) % W]
    assert bool(inside) == (align % W != 0), (lay.block, inside)
    spread(lay.bounds)
    run_and_check(sim, ("chunks", chunks, align), head_start="blocks", poison=True)


@pytest.mark.parametrize("chunks,align", [(3, 1000), (4, 4096)])
def test_chunk_major_layout_on_the_direct_kernel(world_of, chunks, align):
    """The same numbering under pr_step_kernel (no plan: expand() is a no-op, nothing may be poisoned)."""
    n = graph()[0]
    world, bounds = ed.chunk_world(n, chunks)
    sim = world_of(False, world, ("chunks", chunks, "align", align), bounds=bounds, chunks=chunks, align=align)
    run_and_check(sim, ("chunks direct", chunks, align), head_start="blocks")


# ------------------------------------------------------------------------------------------ head start
@pytest.mark.parametrize("align", [1000, 4096])
@pytest.mark.parametrize("head_start", ["twice", "smaller", "zero", "never"])
def test_head_start_variants(world_of, head_start, align):
    """expand() called twice with the same cols_ready, then with a smaller one, preceded by 0, and never (the step
    alone runs all of phase 1): the prover's bits in every variant.  ("blocks", one call per block, is what
    test_chunk_major_layout_with_head_start runs.)  Not-yet-arrived pieces hold NaN in every variant; consumed
    ones are poisoned too wherever a head start was complete."""
    n = graph()[0]
    world, bounds = ed.chunk_world(n, 3)
    sim = world_of(True, world, ("head start", head_start, align), bounds=bounds, chunks=3, align=align)
    run_and_check(sim, ("head start", head_start, align), head_start=head_start, poison=True)


# ------------------------------------------------------------------------------------------ commit forms, push
@pytest.mark.parametrize("tiled", [False, True], ids=["direct", "tiled"])
def test_commit_forms_agree(world_of, tiled):
    """pr_commit_gathered (tails), pr_commit with the pairs added on the host in rank order, and at world 1
    pr_reduce_commit (step_and_commit) and the exchange loop with one rank (tails of a single slice): the prover's
    bits each, and bit-identical states between the two three-rank forms."""
    bounds = ed.equal_row_bounds(graph()[0], 3)
    counts = spread(bounds)
    assert counts.size == 3 and counts.min() > 0 and np.unique(counts).size == 3
    _, _, _, _, steps, trajectory, _, _ = graph()
    forms = [(3, "gather", {}), (3, "sums", {}), (1, "local", {}), (1, "gather", dict(exchange=True))]
    sims = [(world_of(tiled, world, ("commit", mode), **layout), mode) for world, mode, layout in forms]
    for k in range(steps):
        states = []
        for sim, mode in sims:
            sim.step(k, DAMPING, 0.0, mode=mode)
            states.append(sim.check(k, trajectory[k][0], trajectory[k][1], assert_bits, ("commit", mode, tiled)))
        assert states[0] == states[1], states                  # same pairs, same order: the same float


@pytest.mark.parametrize("tiled", [False, True], ids=["direct", "tiled"])
@pytest.mark.parametrize("world", [2, 3])
def test_push_exchange(world_of, world, tiled):
    """spmv_c_pr_step_push: every shard stores its new slice into the peers' vectors as well; the host adds the
    partial pairs (the all-reduce).  Two and three ranks (one and two peers; kMaxPushPeers is 15)."""
    sim = world_of(tiled, world, ("push", world))
    spread(sim.lays[0].bounds)
    run_and_check(sim, ("push", world, tiled), mode="push")


# ------------------------------------------------------------------------------------------ steps after done
@pytest.mark.parametrize("form", ["gather_direct", "gather_tiled_chunks", "push_tiled", "local_tiled"])
def test_steps_after_done_change_nothing(world_of, form):
    """Tolerance just above the prover's residual of step 2 (and below that of step 1): the device sets `done` in
    step 2; two more steps, exchange and head starts included, change no bit of either vector on any rank."""
    _, _, _, _, steps, trajectory, _, _ = graph()
    tolerance = float(np.float32(trajectory[1][1]) * np.float32(1 + 2.0 ** -16))       # 128 ulps above: 4 are allowed
    assert trajectory[1][1] < tolerance < 0.5 * trajectory[0][1]
    n = graph()[0]
    if form == "gather_direct":
        sim, step = world_of(False, 3, form), dict(mode="gather")
    elif form == "gather_tiled_chunks":
        world, bounds = ed.chunk_world(n, 3)
        sim = world_of(True, world, form, bounds=bounds, chunks=3, align=1000)
        step = dict(mode="gather", head_start="blocks")
    elif form == "push_tiled":
        sim, step = world_of(True, 2, form), dict(mode="push")
    else:
        sim, step = world_of(True, 1, form), dict(mode="local")
    sim.step(0, DAMPING, tolerance, **step)
    sim.check(0, trajectory[0][0], trajectory[0][1], assert_bits, form)
    sim.step(1, DAMPING, tolerance, **step)
    state = sim.check(1, trajectory[1][0], trajectory[1][1], assert_bits, form, converged=True)
    before = sim.snapshot()
    for k in (2, 3):
        sim.step(k, DAMPING, tolerance, **step)
    for was, now in zip(before, sim.snapshot()):
        for a, b in zip(was, now):
            assert sim.torch.equal(a, b), form
    assert all(sp.engine.status() == state for sp in sim.loops)


# ------------------------------------------------------------------------------------------ the native loop
def native(gpu, monkeypatch, capfd, shards, options, tiled, through_env, rccl=False):
    """pagerank() with SPMV_NUM_GPUS=shards (or pagerank_multi_gpu(shards) itself) on the graph.

    That the sharded loop produced the result: pagerank() falls back to one device, with a line on stderr, when the
    loop returns nothing (asserted absent), and the loop called directly must exist and agree.  That pagerank() took
    the SPMV_NUM_GPUS route at all is shown where it can be: with `tiled`, SPMV_DEBUG carries pr_plan_after=0, under
    which a one-device pagerank() builds a tiled plan on the caller's matrix from step 0
    (test_pagerank_bit_exact_on_the_tiled_engine), while the sharded loop uploads shards of its own and never touches
    it: the handle must be left WITHOUT a plan.  Without `tiled` a one-device run leaves no such trace, and only the
    two checks above hold.

    What cannot be shown from outside: which engine the loop's own shards ran.  Their headers live inside
    pagerank_multi_gpu, so no csr_tiled_info reaches them.  `tiled` sets the SPMV_DEBUG under which every shard of
    tests/test_gpu_sharded_exact.py's part 1 with at least one tile of rows is ASSERTED to build a plan at (W, R)
    through the same tiled_plan_for; here it is the configuration, not a proved fact.  skip: only with `rccl`."""
    n, rp, ci, va, steps, trajectory, _, _ = graph()
    if tiled:
        monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, "pr_plan_after=0"))
        monkeypatch.setenv("SPMV_TILED_FOLD", "1")
    else:
        monkeypatch.delenv("SPMV_DEBUG", raising=False)
    monkeypatch.setenv("SPMV_MULTI_GPU", options)
    A = pagerank_tests.upload(gpu, rp, ci, va, n)
    try:
        for k in (1, steps):
            config = gpu.PageRankConfig(DAMPING, 0.0, k)
            capfd.readouterr()
            if through_env:
                monkeypatch.setenv("SPMV_NUM_GPUS", str(shards))
                result = gpu.pagerank(A, config)
                monkeypatch.delenv("SPMV_NUM_GPUS")
            else:
                result = gpu.pagerank_multi_gpu(A, config, shards)
            err = capfd.readouterr().err
            if rccl and result.ranks is None and "librccl not available" in err:
                pytest.skip("RCCL cannot be loaded here: " + err.strip())
            assert "[spmv] SPMV_NUM_GPUS=" not in err and "returned nothing" not in err, err
            assert result.ranks is not None, err
            want, residual = trajectory[k - 1]
            print("native", shards, options, "SPMV_DEBUG for tiled shards" if tiled else "direct shards", "steps", k, result.final_residual, residual)
            assert result.iterations == k and not result.converged
            assert_bits(rp, result.ranks, want, ("native", shards, options, tiled, k))
            assert shard_sim.ulps(result.final_residual, residual) <= 4, (result.final_residual, residual)
            if through_env:
                assert not (tiled and gpu.csr_has_tiled_plan(A)), "pagerank() ran on one device"
                # the loop called directly exists and gives the same answer, residual included
                direct = gpu.pagerank_multi_gpu(A, config, shards)
                assert direct.ranks is not None and direct.iterations == k
                assert_bits(rp, direct.ranks, want, ("native direct", shards, options, tiled, k))
                assert direct.final_residual == result.final_residual
    finally:
        gpu.csr_destroy(A)


@pytest.mark.parametrize("tiled", [False, True], ids=["direct", "tiled"])
@pytest.mark.parametrize("blocks", [1, 2, 4])
@pytest.mark.parametrize("shards", [2, 3, 5, 8])
def test_native_loop_through_pagerank(gpu, monkeypatch, capfd, shards, blocks, tiled):
    """csrc/pagerank_multi.cpp: pagerank_shard_bounds, place() / position(), the tails, blocks=C with pr_expand per
    block, the compaction of the result and r /= sum(r) with a sum of exactly 1.0f.  P shards on one device
    (share_devices: the slices travel by device copies)."""
    n, rp = graph()[:2]
    bounds = np.zeros(shards + 1, np.int32)
    import ctypes
    assert gpu.lib().spmv_c_pagerank_shard_bounds(rp.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, shards,
                                                  bounds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    counts = spread(bounds)
    print("native bounds", bounds.tolist(), "dangling per shard", counts.tolist())
    options = "share_devices" + (",blocks=%d" % blocks if blocks > 1 else "")
    native(gpu, monkeypatch, capfd, shards, options, tiled, through_env=True)


@pytest.mark.parametrize("blocks", [1, 3])
def test_native_loop_with_one_shard_through_rccl(gpu, monkeypatch, capfd, blocks):
    """force_rccl keeps tails, blocks and the ncclAllGather in the loop with a single shard.  (pagerank() takes
    SPMV_NUM_GPUS only above 1, so this case calls pagerank_multi_gpu itself.)"""
    options = "force_rccl" + (",blocks=%d" % blocks if blocks > 1 else "")
    native(gpu, monkeypatch, capfd, 1, options, tiled=True, through_env=False, rccl=True)
