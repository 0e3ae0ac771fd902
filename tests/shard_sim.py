"""Row-sharded PageRank on ONE device: the shards of a host CSR matrix as HipEngines, the host playing the exchange.

A plain module (not a test): tests/test_gpu_pagerank.py builds its shards with shard_engine / sharded_loops, and
tests/test_gpu_sharded_exact.py drives the whole loop through Sim, which also holds everything to the bits of the
integer prover (exact_data.dyadic_trajectory) after every step."""
from ctypes import c_void_p

import numpy as np

SENTINEL = 0x7FC0DEAD          # a NaN bit pattern no kernel produces by arithmetic (test_gpu_spmv_multi.SENTINEL)


def shard_engine(prd, torch, dev, rp, ci, va, lay, make_engine=None):
    """HipEngine over rows [lay.row_begin, lay.row_end) of the host CSR (rp, ci, va): row pointers rebased to 0,
    columns renumbered into the padded layout.  `make_engine(row_ptrs, cols, vals, layout)` builds another engine with
    HipEngine's methods from the same arrays (the CPU double of tests/test_distributed_gloo.py)."""
    b, e = lay.row_begin, lay.row_end
    lrp = (rp[b:e + 1] - rp[b]).astype(np.int32)
    lci = lay.remap_columns(ci[rp[b]:rp[e]]).astype(np.int32)
    lva = np.ascontiguousarray(va[rp[b]:rp[e]])
    if make_engine is not None:
        return make_engine(lrp, lci, lva, lay)
    return prd.HipEngine(torch.from_numpy(lrp).to(dev), torch.from_numpy(lci).to(dev), torch.from_numpy(lva).to(dev), lay)


def mask_and_reset(torch, loops):
    """What prepare() and reset() do across ranks: the column sums of all shards added up (the all-reduce), every
    rank's dangling mask from them, the start vector and the start state."""
    dev = loops[0].device
    sums = loops[0].engine.column_sums()
    for sp in loops[1:]:
        sums = sums + sp.engine.column_sums()
    for sp in loops:
        mask = torch.zeros(sp.layout.padded, dtype=torch.uint8, device=dev)
        mask[sp._pos] = (sums[sp._pos] == 0).to(torch.uint8)
        sp.num_dangling = int(mask.sum().item())
        sp.engine.set_dangling_mask(mask)
        sp.reset()


def sharded_loops(prd, torch, dev, rp, ci, va, lays, make_engine=None):
    """One ShardedPageRank per layout of `lays` (the ranks of one world), masks set, vectors and state reset."""
    loops = [prd.ShardedPageRank(shard_engine(prd, torch, dev, rp, ci, va, lay, make_engine), lay) for lay in lays]
    mask_and_reset(torch, loops)
    return loops


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


class Sim:
    """All ranks of one world on one device.  step(k, ...) enqueues iteration k on every rank and plays the exchange;
    check(k, ...) holds every rank to the prover after it.  Padding of the vectors (positions that belong to no node
    and to no tail) is filled with SENTINEL after the reset and must hold it ever after."""

    def __init__(self, gpu, prd, torch, rp, ci, va, n, world, bounds=None, chunks=1, align=None, exchange=None,
                 make_engine=None):
        self.gpu, self.prd, self.torch, self.n, self.world = gpu, prd, torch, n, world
        self.dev = torch.device("cuda:0" if make_engine is None else "cpu")
        self.lays = [prd.Layout(n, world, r, bounds=bounds, chunks=chunks, align=align, exchange=exchange)
                     for r in range(world)]
        lay = self.lays[0]
        self.chunks, self.exchange = lay.chunks, lay.exchange
        self.loops = sharded_loops(prd, torch, self.dev, rp, ci, va, self.lays, make_engine)
        used = np.zeros(lay.padded, bool)
        used[lay.positions()] = True
        for r in range(world if lay.exchange else 0):
            used[lay.tail_slice(r)] = True
        self.free = torch.from_numpy(np.flatnonzero(~used)).to(self.dev)
        for sp in self.loops:
            for buf in sp.r:
                buf.view(torch.int32)[self.free] = SENTINEL
        self.rp = rp

    # ---- what ran
    def describe(self):
        lay = self.lays[0]
        plans = []
        for sp in self.loops:
            info = self.gpu.csr_tiled_info(sp.engine._A) if self.gpu.csr_has_tiled_plan(sp.engine._A) else None
            plans.append(None if info is None else (info["strip_cols"], info["tile_rows"], info["num_strips"],
                                                    info["num_tiles"], info["long_rows"]))
        return dict(world=self.world, bounds=[int(b) for b in lay.bounds], chunks=lay.chunks, piece=lay.piece,
                    block=lay.block, padded=lay.padded, exchange=lay.exchange,
                    nnz=[int(sp.engine._keep[1].numel()) for sp in self.loops], plans_W_R_strips_tiles_long=plans)

    def assert_engines(self, tiled, W=None, R=None, long_rows_somewhere=True):
        """Every shard of at least one full tile of rows runs the tiled engine at (W, R) when `tiled` (smaller ones
        with entries may: describe() prints what they got; without entries none can), no shard has a plan otherwise."""
        longs = 0
        for sp in self.loops:
            has = bool(self.gpu.csr_has_tiled_plan(sp.engine._A))
            nnz = int(sp.engine._keep[1].numel())
            assert not has or (tiled and nnz > 0), (sp.layout.rank, has, nnz)
            assert has or not (tiled and sp.layout.local_rows >= R and nnz > 0), (sp.layout.rank, has, nnz)
            if has:
                info = self.gpu.csr_tiled_info(sp.engine._A)
                assert (info["strip_cols"], info["tile_rows"]) == (W, R), info
                assert info["num_strips"] == -(-sp.layout.padded // W), info
                longs += info["long_rows"]
        assert not (tiled and long_rows_somewhere) or longs >= 1, longs      # a hub row: the long-row path is in use

    # ---- one iteration
    def bufs(self, k):
        return [sp.r[k & 1] for sp in self.loops], [sp.r[(k + 1) & 1] for sp in self.loops]

    def _gather_piece(self, news, c):
        for src in range(self.world):
            sl = self.lays[src].piece_slice(c, src)
            for dst in range(self.world):
                if dst != src:
                    news[dst][sl] = news[src][sl]

    def _poison(self, bufs, value=float("nan")):
        for me in range(self.world):
            for other in range(self.world):
                if other != me:
                    for c in range(self.chunks):
                        bufs[me][self.lays[me].piece_slice(c, other)] = value

    def step(self, k, damping, tolerance, mode="gather", head_start="blocks", poison=False):
        """mode: "gather" (tails + commit_gathered), "sums" (the partial pairs added on the host in rank order +
        commit), "push" (step_push into the peers' vectors + commit), "local" (world 1 without exchange:
        step_and_commit).  head_start (chunks > 1): "blocks" = expand() as each block arrives, "twice" = every such
        call made twice, "smaller" = each followed by one with fewer columns, "zero" = each preceded by expand(0),
        "never" = no expand at all.  poison: foreign pieces hold NaN wherever the engine must not look (not yet
        arrived; already consumed by a complete head start)."""
        torch = self.torch
        olds, news = self.bufs(k)
        consumed = self.chunks > 1 and head_start != "never" and k > 0
        if mode == "local":
            assert self.world == 1 and not self.exchange
            self.loops[0].engine.step_and_commit(olds[0], news[0], damping, tolerance)
            return
        if poison and consumed:
            self._poison(olds)
        partial = []
        for me, sp in enumerate(self.loops):
            if mode == "gather":
                sp.engine.step(olds[me], news[me], damping, sp._my_tail(news[me]))
            elif mode == "sums":
                partial.append(sp.engine.step(olds[me], news[me], damping).clone())
            else:
                peers = [news[q].data_ptr() for q in range(self.world) if q != me]
                partial.append(sp.engine.step(olds[me], news[me], damping,
                                              push_to=(c_void_p * len(peers))(*peers)).clone())
        if mode != "push":
            if poison:
                self._poison(news)
            for c in range(self.chunks):
                self._gather_piece(news, c)
                if self.chunks > 1 and head_start != "never":
                    ready = (c + 1) * self.lays[0].block
                    for me, sp in enumerate(self.loops):
                        if head_start == "zero":
                            sp.engine.expand(news[me], 0)
                        sp.engine.expand(news[me], ready)
                        if head_start == "twice":
                            sp.engine.expand(news[me], ready)
                        if head_start == "smaller":
                            sp.engine.expand(news[me], ready - self.lays[0].block)
        if mode == "gather":
            for me, sp in enumerate(self.loops):
                sp.engine.commit_gathered(news[me], tolerance)
        else:
            total = torch.zeros(2, dtype=torch.float64, device=self.dev)
            for p in partial:                                   # rank order, as pr_commit_gathered_kernel folds
                total = total + p
            for sp in self.loops:
                sp.engine.commit(total, tolerance)

    # ---- the checks after iteration k (0-based)
    def check(self, k, want, residual, assert_bits, what, converged=False, tails=True):
        torch = self.torch
        _, news = self.bufs(k)
        first = news[0].view(torch.int32)
        for me, sp in enumerate(self.loops):
            got = news[me][sp._pos].cpu().numpy()
            assert_bits(self.rp, got, want, (what, "step", k + 1, "rank", me))
            mine = news[me].view(torch.int32)
            assert bool((mine[self.free] == SENTINEL).all()), (what, "padding written", k + 1, me)
            if tails:                                           # the whole vector, tails included, on every rank
                assert torch.equal(mine, first), (what, "rank vectors differ", k + 1, me)
        states = [sp.engine.status() for sp in self.loops]
        assert all(s == states[0] for s in states), (what, states)
        iterations, got_residual, conv, done = states[0]
        assert (iterations, conv, done) == (k + 1, converged, converged), (what, states[0])
        assert ulps(got_residual, residual) <= 4, (what, k + 1, got_residual, residual)
        return states[0]

    def snapshot(self):
        return [[buf.view(self.torch.int32).clone() for buf in sp.r] for sp in self.loops]

    def close(self):
        for sp in self.loops:
            if hasattr(sp.engine, "close"):
                sp.engine.close()
            sp.close()
