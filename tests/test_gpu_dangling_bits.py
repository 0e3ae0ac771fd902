"""The tiled engine's phase 2 reads the dangling flags of a contiguous slice as BITS, one per local row, derived from
the caller's byte mask when the shard is created and again by every spmv_c_pr_reset, and skips them for a tile
without a dangling row (DanglingBits, csrc/pagerank_engine.h; tiled_pagerank_reduce_kernel, csrc/tiled.hip).

Part 1, against the integer prover (exact_data.dyadic_trajectory, as tests/test_gpu_sharded_exact.py): n = 4096,
R = 64, damping 0.5, three exact steps, so the mass the device accumulated over the flagged rows in step k is the
dangling term of step k + 1 under a bit-exact comparison; the state's dangling_sum is compared with the prover's too.
  graph A   dangling nodes at rows 0, R - 1, R and n - 1, every row of tile 5 (tile 4 and tile 6 have none) and 60
            rows of tile 20: one shard; two shards cut at row 1001 (1001 and 3095 local rows: no multiple of 32, a
            last tile of 41 and of 23 rows, the second shard's bits counted from ITS first row, at position 3100 of the vector); and two
            shards on a chunk-major vector, where the mapped branch keeps reading bytes.
  graph B   every node of the second shard dangling (columns 2048 .. 4095 without entries), none of the first.
Part 2, on data that are not exact (n = 20 011: no multiple of 32, a last tile of 43 rows): the bits and the bytes
(SPMV_DEBUG=dangling=bytes) run the same operations in the same order, so ranks, residual and dangling mass agree
bit for bit after every one of five steps, and so do two resets of one shard."""
import importlib
from ctypes import byref

import numpy as np
import pytest

import exact_data as ed
import shard_sim

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
assert_bits = sweep.assert_bits
N, W, R, DAMPING = 4096, 4096, 64, ed.DYADIC_DAMPING
_graphs = {}


def graph(name):
    """(rp, ci, va, dangling nodes, [(ranks, residual)] of the exact steps)"""
    if name not in _graphs:
        if name == "A":
            dangling = np.unique(np.concatenate([[0, R - 1, R, N - 1], np.arange(5 * R, 6 * R), np.arange(20 * R, 20 * R + 60)]))
            rng = np.random.default_rng(11)
        else:
            dangling = np.arange(N // 2, N)
            rng = np.random.default_rng(12)
        assert dangling.size & (dangling.size - 1) == 0
        rp, ci, va = ed.dyadic_graph(rng, N, (2, 4), dangling, [])
        steps = ed.exact_steps(rp, ci, va, N, DAMPING)
        assert steps >= 3, steps
        assert np.array_equal(np.flatnonzero(np.bincount(ci, minlength=N) == 0), dangling)
        _graphs[name] = (rp, ci, va, dangling, ed.dyadic_trajectory(rp, ci, va, N, DAMPING, steps))
    return _graphs[name]


def dangling_sum(gpu, sp):
    out = gpu.PrStatus()
    assert gpu.lib().spmv_c_pr_status_get(sp.engine._shard, byref(out), sp.engine._stream()) == 0
    return np.float32(out.dangling_sum)


def run_exact(gpu, monkeypatch, name, fold, world, what, **layout):
    torch = pytest.importorskip("torch")
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    rp, ci, va, dangling, trajectory = graph(name)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R))
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if fold else "0")
    sim = shard_sim.Sim(gpu, prd, torch, rp, ci, va, N, world, **layout)
    try:
        sim.assert_engines(True, W, R, long_rows_somewhere=False)
        assert all(gpu.csr_has_tiled_plan(sp.engine._A) for sp in sim.loops), sim.describe()
        print(what, sim.describe())
        for k, (ranks, residual) in enumerate(trajectory):
            sim.step(k, DAMPING, 0.0, mode="local" if world == 1 else "gather")
            sim.check(k, ranks, residual, assert_bits, (what, fold))
            want_mass = np.float32(ranks[dangling].astype(np.float64).sum())       # dyadic and short: the sum is exact
            for sp in sim.loops:
                assert dangling_sum(gpu, sp).view(np.uint32) == want_mass.view(np.uint32), (what, k, sp.layout.rank)
    finally:
        sim.close()


@pytest.mark.parametrize("fold", [False, True], ids=["stream", "fold"])
def test_flags_at_tile_edges_and_a_full_tile_beside_an_empty_one(gpu, monkeypatch, fold):
    run_exact(gpu, monkeypatch, "A", fold, 1, "one shard")


def test_two_shards_whose_rows_are_no_multiple_of_32(gpu, monkeypatch):
    run_exact(gpu, monkeypatch, "A", False, 2, "cut at 1001", bounds=[0, 1001, N])


def test_every_node_of_a_shard_dangling_beside_a_shard_with_none(gpu, monkeypatch):
    run_exact(gpu, monkeypatch, "B", True, 2, "all and none")


def test_chunk_major_vector_keeps_the_byte_mask(gpu, monkeypatch):
    run_exact(gpu, monkeypatch, "A", False, 2, "mapped branch", chunks=2)


# ------------------------------------------------------------------------------------------ bits against bytes
AB_N, AB_K, AB_STEPS = 20011, 8, 5


def ab_graph(spmv):
    rp, ci, _ = spmv.synth.uniform_csr(5, 0, AB_N, AB_N, AB_K)
    T = -(-AB_N // R)
    dangling = np.unique(np.concatenate([[0, R - 1, R, AB_N - 1], np.arange(3 * R, 4 * R), np.arange((T - 1) * R, AB_N, 3)]))
    keep = ~np.isin(ci, dangling)
    rows = np.repeat(np.arange(AB_N), np.diff(rp))[keep]
    ci = np.ascontiguousarray(ci[keep])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=AB_N))]).astype(np.int32)
    va = spmv.synth.column_stochastic_values(ci, AB_N)
    return rp, ci, va, dangling


def ab_run(gpu, monkeypatch, extra, resets):
    torch = pytest.importorskip("torch")
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    rp, ci, va, dangling = ab_graph(gpu)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, R, extra))
    monkeypatch.setenv("SPMV_TILED_FOLD", "0")
    dev = torch.device("cuda:0")
    lay = prd.Layout(AB_N)
    eng = prd.HipEngine(torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(va).to(dev), lay)
    sp = prd.ShardedPageRank(eng, lay).prepare()
    out = []
    try:
        info = gpu.csr_tiled_info(eng._A)
        assert info is not None and (info["strip_cols"], info["tile_rows"]) == (W, R), info
        mask = eng._mask.cpu().numpy()
        assert set(np.flatnonzero(mask[:AB_N])) >= set(dangling) and mask[4 * R:5 * R].sum() == 0 and mask[3 * R:4 * R].all()
        for _ in range(resets):
            sp.reset()
            for k in range(AB_STEPS):
                eng.step_and_commit(sp.r[k & 1], sp.r[(k + 1) & 1], 0.85, 0.0)
                status = eng.status()
                out.append((sp.r[(k + 1) & 1][:AB_N].cpu().numpy().view(np.uint32).copy(), status,
                            int(dangling_sum(gpu, sp).view(np.uint32))))
                assert status[0] == k + 1
    finally:
        eng.close()
        sp.close()
    return out


def test_bits_and_bytes_agree_bit_for_bit_on_inexact_data(gpu, monkeypatch):
    bits = ab_run(gpu, monkeypatch, "", resets=2)
    bytes_ = ab_run(gpu, monkeypatch, "dangling=bytes", resets=1)
    assert len(bits) == 2 * AB_STEPS and len(bytes_) == AB_STEPS
    for k in range(AB_STEPS):
        for run in (bits[k], bits[AB_STEPS + k]):                    # the second reset derives the bits again
            np.testing.assert_array_equal(run[0], bytes_[k][0], err_msg="ranks after step %d" % (k + 1))
            assert run[1] == bytes_[k][1] and run[2] == bytes_[k][2], (k, run[1:], bytes_[k][1:])
    assert bytes_[AB_STEPS - 1][2] != 0 and not np.array_equal(bytes_[0][0], bytes_[1][0])
