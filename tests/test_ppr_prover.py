"""The integer prover of personalized PageRank (tests/ppr_cases.py), without a GPU: the floors that keep the exact GPU
cases of tests/test_gpu_ppr.py from being vacuous, and agreement with exact_data's prover of pagerank() where the two
overlap (v = 1 / n)."""
import numpy as np
import pytest

import exact_data as ed
import ppr_cases as pc


@pytest.mark.parametrize("degrees", pc.DEGREES, ids=lambda d: "deg" + "_".join(map(str, d)))
def test_seeded_sets_stay_exact_for_the_stated_number_of_steps(degrees):
    """Every set of the catalogue (a node, a dangling node, a hub, a pair, eight nodes) on every graph: at least six
    exact steps with out-degrees up to 8, four with (16, 32); the residual the device reports is provable for all of
    them; the graphs land on the lane counts 1, 1, 2 and 8."""
    rp, ci, va = pc.graph(degrees)
    counts = [pc.exact_steps(rp, ci, va, pc.N, s, pc.DAMPING, 10) for s in pc.seed_sets()]
    print(degrees, "exact steps per set", counts, "lanes", ed.lanes_for(len(ci), pc.N))
    assert min(counts) >= pc.FLOORS[degrees] >= 4, counts
    steps, trajectories = pc.proven(degrees)
    assert steps == min(min(counts), 8) and all(len(t) == steps for t in trajectories)
    for t in trajectories:
        for ranks, residual, reported in t:
            assert ranks.dtype == np.float32 and float(ranks.astype(np.float64).sum()) == 1.0
            assert abs(float(reported) - residual) <= 2.0 ** -22 * residual


def test_the_ranks_spread_over_most_of_the_graph():
    """(4, 8) from node 17: about 1 880 of the 2 048 nodes carry rank after six steps, so the exact comparison covers
    rows of every length, the hubs included."""
    rp, ci, va = pc.graph((4, 8))
    reached = [int((ranks > 0).sum()) for ranks, _, _ in pc.trajectory(rp, ci, va, pc.N, [17], pc.DAMPING, 6)]
    print("nodes with rank after each step", reached)
    assert reached == sorted(reached) and reached[-1] >= 1800
    assert np.diff(rp)[pc.N // 3] == 1500 and np.diff(rp)[pc.N - 1] == 600


def test_the_dangling_seed_and_the_dangling_mass():
    """Node 3 is dangling: its column is v after every step (A v = 0, s = 1), residual 0.  The other sets lose mass to
    the dangling nodes from some step on, so the device-accumulated mass enters an exact step."""
    rp, ci, va = pc.graph((2, 4))
    dangling = np.bincount(ci, minlength=pc.N) == 0
    assert dangling[3] and sorted(np.flatnonzero(dangling)) == sorted(ed.DYADIC_DIRECT_DANGLING)
    for ranks, residual, reported in pc.trajectory(rp, ci, va, pc.N, [3], pc.DAMPING, 4):
        assert ranks[3] == 1.0 and residual == 0.0 and reported == 0.0
    steps, trajectories = pc.proven((2, 4))
    masses = [[float(ranks[dangling].sum()) for ranks, _, _ in t] for t in trajectories]
    print("dangling mass per set and step", masses)
    assert any(m > 0 for m in masses[0][:steps - 1]) and any(m > 0 for m in masses[4][:steps - 1])


@pytest.mark.parametrize("degrees", pc.DEGREES, ids=lambda d: "deg" + "_".join(map(str, d)))
def test_uniform_teleport_agrees_with_the_pagerank_prover(degrees):
    """v = 1 / n: the same exact-step count as exact_data.exact_steps (one or two: the uniform vector fills every
    row at once) and dyadic_pagerank's ranks and residual, step by step."""
    rp, ci, va = pc.graph(degrees)
    everyone = np.arange(pc.N)
    mine = pc.exact_steps(rp, ci, va, pc.N, everyone, pc.DAMPING, 4, with_residual=False)
    theirs = ed.exact_steps(rp, ci, va, pc.N, pc.DAMPING, 4)
    print(degrees, "exact steps with v = 1/n", mine, theirs)
    assert mine == theirs and 1 <= mine <= 3
    got = pc.trajectory(rp, ci, va, pc.N, everyone, pc.DAMPING, 3)
    want = ed.dyadic_trajectory(rp, ci, va, pc.N, pc.DAMPING, 3)
    for (ranks, residual, _), (ranks_ref, residual_ref) in zip(got, want):
        assert np.array_equal(ranks.view(np.uint32), ranks_ref.view(np.uint32)) and residual == residual_ref


def test_the_float64_iteration_reproduces_an_exact_trajectory():
    """power_iteration64 on a dyadic graph for the proven number of steps: dyadic arithmetic is exact in float64 too."""
    degrees = (4, 8)
    rp, ci, va = pc.graph(degrees)
    steps, trajectories = pc.proven(degrees)
    V = pc.teleport_matrix(pc.N, pc.seed_sets())
    R, iterations, residuals, converged = pc.power_iteration64(rp, ci, va, pc.N, V, pc.DAMPING, 0.0, steps)
    assert iterations == [steps] * 5 and not any(converged)
    for j, t in enumerate(trajectories):
        assert np.array_equal(R[:, j].astype(np.float32).view(np.uint32), t[-1][0].view(np.uint32))
        assert residuals[j][-1] == t[-1][1]
