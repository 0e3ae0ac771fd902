"""The two ends of a workgroup's life in the tiled PageRank step (csrc/tiled.hip).  Phase 2 asks for `done`, the
dangling mass, the tile's flagged-row count and the wavefront's pass range together, in front of the cleared tile, and
its contiguous-slice branch stores r_new non-temporally; two more moves of loads were measured and are not in the code
(phase 1's item record together with `done`; a thread's r_old values and flag words in front of the barrier that
closes the tile — profiles/step_ends_ab.txt), and these tests are where such a move would show.  None of it may change
a bit: exact dyadic graphs (exact_data.dyadic_graph) against the integer prover after every step, through the shard
simulator of tests/test_gpu_sharded_exact.py.

n = 16384, W = 4096 (four strips and more), damping 0.5.  What can go wrong with a moved load shows where it is clamped
or skipped:
  * a last tile with rows_here < R at R = 64 (one row per thread: shards of 1001 and 15383 rows, last tiles of 41
    and 23 rows) and at R = 9984 (ten rows per thread: a second tile of 6400 rows) — with dangling rows in the short
    tiles, in full tiles only, and nowhere (flagged tiles, unflagged tiles, and a shard whose every count is zero);
    the byte mask (SPMV_DEBUG=dangling=bytes) rides along on the first of them;
  * shards of 1 and of 65 local rows;
  * steps enqueued past convergence through the deferred commit (spmv_c_pr_step_commit): five steps with a tolerance
    that step 2 meets leave both rank vectors and the status as two steps and a status call do.  (The product
    scratch is not compared: no call reads it, and phase 1 of step 3 may or may not have rewritten it before the
    commit riding in the same launch set `done` — the kernel's comment argues why either is right.)
  * hub rows beyond the long-row limit, all steps enqueued without a status call in between, so that the head of
    every phase-1 grid after the first is commit workgroups, then long-row workgroups, then items;
  * rank vectors that are views four bytes past a 16-byte boundary (and 12 past) into larger buffers whose other
    elements must keep their bits;
  * the chunk-major vector (mapped branch: untouched code) on the same graph."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import shard_sim

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
assert_bits = sweep.assert_bits
N, W, DAMPING = 1 << 14, 4096, ed.DYADIC_DAMPING
SHORT_CUT = 1001                                   # shards of 1001 and N - 1001 rows: last tiles of 41 and 23 rows at R = 64
BIG_R = 9984                                       # tiles of 9984 and 6400 rows
HUBS = [(N // 3, 700), (N - 1, 350)]               # beyond the long-row limit (8 per strip)
DANGLING_COUNT = 256                               # a power of two, and enough of them: d * s / n stays short for two steps
KEYS = [(R, where) for R in (64, BIG_R) for where in ("short", "full", "none")]
_graphs = {}


def in_short_tile(R, nodes):
    if R == 64:
        return ((nodes >= SHORT_CUT // 64 * 64) & (nodes < SHORT_CUT)) | (nodes >= SHORT_CUT + (N - SHORT_CUT) // 64 * 64)
    return nodes >= BIG_R


def dangling_nodes(rng, key, hubs):
    """DANGLING_COUNT nodes that dyadic_graph links from nowhere (row % 13 == 5: exact_data.source_only_nodes — their
    ranks stay short beyond the first step).  "short": every such node of the short last tiles (four at R = 64: three of
    the first shard's, one of the second's; at R = 9984 the second tile holds all 256, the full tile none), the rest
    elsewhere; "full": none of them in a short tile."""
    R, where = key
    if where == "none":
        return np.zeros(0, np.int64)
    nodes = ed.source_only_nodes(N, list(hubs))
    short = in_short_tile(R, nodes)
    first = nodes[short] if where == "short" else nodes[:0]
    if first.size > DANGLING_COUNT:                             # spread over the tile, its first and last such node included
        first = first[np.linspace(0, first.size - 1, DANGLING_COUNT).astype(np.int64)]
    assert where != "short" or (first.size >= 4 and first[-1] >= N - 23)
    rest = rng.choice(nodes[~short], size=DANGLING_COUNT - first.size, replace=False)
    return np.sort(np.concatenate([first, rest]))


def graph(key, hubs=()):
    """(rp, ci, va, dangling, [(ranks, residual)] of the exact steps, at least two)"""
    name = (key, tuple(hubs))
    if name not in _graphs:
        rng = np.random.default_rng(700 + KEYS.index(key) + 50 * len(hubs))
        dangling = dangling_nodes(rng, key, hubs)
        rp, ci, va = ed.dyadic_graph(rng, N, (2, 4), dangling, list(hubs))
        steps = ed.exact_steps(rp, ci, va, N, DAMPING)
        assert steps >= 2, (key, steps)
        assert np.array_equal(np.flatnonzero(np.bincount(ci, minlength=N) == 0), np.sort(dangling))
        _graphs[name] = (rp, ci, va, dangling, ed.dyadic_trajectory(rp, ci, va, N, DAMPING, steps))
    return _graphs[name]


def exact_run(gpu, monkeypatch, g, R, world, what, extra="", plans=None, **layout):
    """Every exact step on `world` shards, each held to the prover after it (ranks bit for bit, residual, padding)."""
    torch = pytest.importorskip("torch")
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    rp, ci, va, dangling, trajectory = g
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, extra))
    monkeypatch.setenv("SPMV_TILED_FOLD", "0")
    sim = shard_sim.Sim(gpu, prd, torch, rp, ci, va, N, world, **layout)
    try:
        print(what, sim.describe())
        for sp in sim.loops if plans is None else [sim.loops[r] for r in plans]:
            assert gpu.csr_has_tiled_plan(sp.engine._A), (what, sp.layout.rank)
            info = gpu.csr_tiled_info(sp.engine._A)
            assert (info["strip_cols"], info["tile_rows"]) == (W, R), info
        for k, (ranks, residual) in enumerate(trajectory):
            sim.step(k, DAMPING, 0.0, mode="local" if world == 1 else "gather")
            sim.check(k, ranks, residual, assert_bits, what)
    finally:
        sim.close()
    return sim


@pytest.mark.parametrize("where", ["short", "full", "none"])
def test_short_last_tile_one_row_per_thread(gpu, monkeypatch, where):
    exact_run(gpu, monkeypatch, graph((64, where)), 64, 2, ("R 64", where), bounds=[0, SHORT_CUT, N])


def test_short_last_tile_with_the_byte_mask(gpu, monkeypatch):
    exact_run(gpu, monkeypatch, graph((64, "short")), 64, 2, "R 64 bytes", extra="dangling=bytes", bounds=[0, SHORT_CUT, N])


@pytest.mark.parametrize("where", ["short", "full", "none"])
def test_short_last_tile_ten_rows_per_thread(gpu, monkeypatch, where):
    sim = exact_run(gpu, monkeypatch, graph((BIG_R, where)), BIG_R, 1, ("R 9984", where))
    assert N - BIG_R < BIG_R and sim.lays[0].local_rows == N


def test_shards_of_one_and_of_65_rows(gpu, monkeypatch):
    g = graph((64, "full"), hubs=[(0, 6)])                       # row 0 has entries: the one-row shard gets a plan
    assert g[0][1] - g[0][0] >= 6 and g[0][66] - g[0][1] > 0
    sim = exact_run(gpu, monkeypatch, g, 64, 3, "1 / 65 / rest", bounds=[0, 1, 66, N])
    assert [lay.local_rows for lay in sim.lays] == [1, 65, N - 66]


def test_chunk_major_vector_still_matches(gpu, monkeypatch):
    exact_run(gpu, monkeypatch, graph((64, "short")), 64, 2, "mapped branch", chunks=2)


# ------------------------------------------------------------------ one shard driven by hand: step_commit, no status between
class Single:
    """One shard of the whole graph; the rank vectors are the loop's own or views `offsets` elements into larger buffers."""

    def __init__(self, gpu, monkeypatch, g, R, offsets=None):
        self.torch = torch = pytest.importorskip("torch")
        prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
        rp, ci, va = g[:3]
        monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
        monkeypatch.setenv("SPMV_TILED_FOLD", "0")
        dev = torch.device("cuda:0")
        self.lay = prd.Layout(N)
        self.eng = prd.HipEngine(torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(va).to(dev), self.lay)
        self.sp = prd.ShardedPageRank(self.eng, self.lay).prepare()
        self.info = gpu.csr_tiled_info(self.eng._A)
        assert self.info is not None and (self.info["strip_cols"], self.info["tile_rows"]) == (W, R), self.info
        self.big = None
        if offsets is not None:
            pad = self.lay.padded
            self.big = [torch.full((pad + 16,), shard_sim.SENTINEL, dtype=torch.int32, device=dev) for _ in offsets]
            base = [(-b.data_ptr() // 4) % 4 for b in self.big]          # elements up to the next 16-byte boundary
            self.at = [b0 + off for b0, off in zip(base, offsets)]
            self.own = self.sp.r
            self.sp.r = [b.view(torch.float32)[a:a + pad] for b, a in zip(self.big, self.at)]
            assert [v.data_ptr() % 16 for v in self.sp.r] == [4 * off for off in offsets]

    def run(self, steps, tolerance):
        """reset, `steps` deferred-commit steps, ONE status call -> (both vectors' bits, status)"""
        self.sp.reset()
        for k in range(steps):
            self.eng.step_and_commit(self.sp.r[k & 1], self.sp.r[(k + 1) & 1], DAMPING, tolerance)
        status = self.eng.status()
        self.torch.cuda.synchronize()
        return [v[:N].cpu().numpy().copy() for v in self.sp.r], (status[0], np.float32(status[1]).view(np.uint32), status[2], status[3])

    def close(self):
        if self.big is not None:
            self.sp.r = self.own
        self.eng.close()
        self.sp.close()


def test_long_rows_commit_rider_and_items_in_one_launch(gpu, monkeypatch):
    g = graph((64, "full"), hubs=HUBS)
    s = Single(gpu, monkeypatch, g, 64)
    try:
        assert s.info["long_rows"] == len(HUBS), s.info
        steps = len(g[4])
        vectors, status = s.run(steps, 0.0)
        assert status[0] == steps and not status[3], status
        assert_bits(g[0], vectors[steps & 1], g[4][steps - 1][0], "last step")
        assert_bits(g[0], vectors[(steps - 1) & 1], g[4][steps - 2][0], "the step before")
        assert shard_sim.ulps(np.uint32(status[1]).view(np.float32), g[4][steps - 1][1]) <= 4
    finally:
        s.close()


@pytest.mark.parametrize("R", [64, BIG_R])
def test_steps_enqueued_past_convergence(gpu, monkeypatch, R):
    g = graph((R, "short"), hubs=HUBS)
    first, second = g[4][0][1], g[4][1][1]
    assert second < first
    tolerance = float(np.float32((first + second) / 2))
    assert second * (1 + 1e-5) < tolerance < first * (1 - 1e-5)           # clear of the residual's four ulps
    s = Single(gpu, monkeypatch, g, R)
    try:
        stopped_vectors, stopped = s.run(2, tolerance)
        assert stopped[0] == 2 and stopped[2] and stopped[3], stopped
        vectors, status = s.run(5, tolerance)
        assert status == stopped, (status, stopped)
        for got, want in zip(vectors, stopped_vectors):
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        assert_bits(g[0], vectors[0], g[4][1][0], "step 2")
        assert_bits(g[0], vectors[1], g[4][0][0], "step 1")
    finally:
        s.close()


@pytest.mark.parametrize("R", [64, BIG_R])
def test_rank_vectors_that_are_views_four_bytes_past_alignment(gpu, monkeypatch, R):
    g = graph((R, "short"))
    s = Single(gpu, monkeypatch, g, R, offsets=(1, 3))
    try:
        steps = len(g[4])
        vectors, status = s.run(steps, 0.0)
        assert status[0] == steps, status
        assert_bits(g[0], vectors[steps & 1], g[4][steps - 1][0], "last step")
        assert_bits(g[0], vectors[(steps - 1) & 1], g[4][steps - 2][0], "the step before")
        pad = s.lay.padded
        for big, at in zip(s.big, s.at):
            outside = np.concatenate([big[:at].cpu().numpy(), big[at + pad:].cpu().numpy()])
            assert outside.size == 16 and (outside == shard_sim.SENTINEL).all(), outside
    finally:
        s.close()
