"""The deferred residual commit (spmv_c_pr_step_commit): on the tiled engine the commit of step k rides in one
workgroup at the head of step k + 1's phase-1 launch, and anything else that comes next on the shard flushes it as
a launch of its own.  Every test compares with the three-launch form (spmv_c_pr_step + spmv_c_pr_reduce_commit)
BIT FOR BIT: both run the same device function on the same block partials.

Small matrices (20 000 x 20 000, 8 per row; one of them with three rows beyond the long-row limit, so that the head
of the phase-1 grid holds long-row workgroups AND the commit workgroup) go through the tiled engine with
SPMV_DEBUG=min_cols=1,min_nnz=1,strip=4096,tile=1024 (5 strips, 20 tiles).  The thresholds are read once per
process, so the device work runs in a worker process — this file itself, started once for the whole module; it
prints one JSON line with the outcome of every scenario.  The engine switch of pagerank() needs two more
environments (pr_plan_after=2; SPMV_TILED=0), one short worker each.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N, K, STEPS, DAMPING = 20_000, 8, 12, 0.85
STOP_AT = 6                       # scenario "convergence": the tolerance is put between the residuals of steps 5 and 6
SWITCH_N, SWITCH_K = 100_000, 12  # pagerank() takes the tiled engine by itself from 32769 columns and 2^20 entries


# ------------------------------------------------------------------------------------------ worker side ----
class Bench:
    """One matrix on the device, its shard engine and the two rank vectors; steps in either form."""

    def __init__(self, spmv, prd, torch, rp, ci, va, fold):
        os.environ["SPMV_TILED_FOLD"] = "1" if fold else "0"
        self.spmv, self.torch, self.lib = spmv, torch, spmv.lib()
        dev = torch.device("cuda:0")
        self.lay = prd.Layout(N)
        self.eng = prd.HipEngine(torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev),
                                 torch.from_numpy(va).to(dev), self.lay)
        self.pr = prd.ShardedPageRank(self.eng, self.lay).prepare()
        self.info = spmv.csr_tiled_info(self.eng._A)
        assert self.info is not None and self.info["num_strips"] > 1 and self.info["num_tiles"] > 1, self.info

    def _stream(self):
        return self.eng._stream()

    def _ptrs(self, k):
        from ctypes import c_void_p
        return c_void_p(self.pr.r[k & 1].data_ptr()), c_void_p(self.pr.r[(k + 1) & 1].data_ptr())

    def plain_step(self, k):
        old, new = self._ptrs(k)
        assert self.lib.spmv_c_pr_step(self.eng._shard, old, new, DAMPING, self._stream()) == 0

    def reduce_commit(self, tol):
        assert self.lib.spmv_c_pr_reduce_commit(self.eng._shard, tol, self._stream()) == 0

    def old_step(self, k, tol):
        self.plain_step(k)
        self.reduce_commit(tol)

    def new_step(self, k, tol):
        old, new = self._ptrs(k)
        assert self.lib.spmv_c_pr_step_commit(self.eng._shard, old, new, DAMPING, tol, self._stream()) == 0

    def status(self):
        from ctypes import byref
        out = self.spmv.PrStatus()
        assert self.lib.spmv_c_pr_status_get(self.eng._shard, byref(out), self._stream()) == 0
        return status_tuple(out)

    def bits(self, which):
        return self.pr.r[which].clone()          # a copy on the same stream: touches neither the shard nor its state

    def both(self):
        self.torch.cuda.synchronize()
        return [self.pr.r[w].cpu().numpy().view(np.uint32).copy() for w in (0, 1)]

    def run(self, step, tol, steps=STEPS, status_each=False):
        """reset, `steps` steps; -> (vector written by every step, status after every step or only the last)."""
        self.pr.reset()
        vectors, states = [], []
        for k in range(steps):
            step(k, tol)
            vectors.append(self.bits((k + 1) & 1))
            if status_each:
                states.append(self.status())
        if not status_each:
            states.append(self.status())
        self.torch.cuda.synchronize()
        return [v.cpu().numpy().view(np.uint32) for v in vectors], states

    def close(self):
        self.pr.close()
        self.eng.close()


def status_tuple(out):
    return (int(out.iterations), int(np.float32(out.final_residual).view(np.uint32)), int(out.converged), int(out.done))


def same_vectors(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        bad = int(np.count_nonzero(x != y))
        assert bad == 0, "%s: %d of %d values differ in vector %d" % (what, bad, x.size, k)


def matrices(spmv):
    """(name, row_ptrs, cols, values, fold): uniform with a few dangling nodes on the value stream (the path
    bench.py quotes); three long rows and dangling nodes through the folded plan."""
    out = []
    rp, ci, _ = spmv.synth.uniform_csr(91, 0, N, N, K)
    keep = ~np.isin(ci, np.array([3, 4097, 19_999], dtype=np.int32))          # columns without entries: dangling nodes
    counts = np.add.reduceat(keep.astype(np.int64), rp[:-1])
    ci = ci[keep]
    rp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out.append(("uniform", rp, ci, spmv.synth.column_stochastic_values(ci, N), False))
    lens = np.full(N, K, dtype=np.int64)
    lens[[7, 9_000, 19_998]] = (3000, 1500, 5000)                              # beyond the long-row limit (1024)
    rp, ci, _ = spmv.synth.stratified_csr(92, 0, lens, N)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    out.append(("long_rows", rp, ci, spmv.synth.column_stochastic_values(ci, N), True))
    return out


def scenario_bit_equality(b, ref):
    vectors, states = b.run(b.new_step, 0.0, status_each=True)
    same_vectors(vectors, ref["vectors"], "status after every step")
    assert states == ref["states"], ("status after every step", states, ref["states"])
    assert [s[0] for s in states] == list(range(1, STEPS + 1))
    vectors, states = b.run(b.new_step, 0.0, status_each=False)
    same_vectors(vectors, ref["vectors"], "status at the end only")
    assert states == ref["states"][-1:], ("status at the end only", states, ref["states"][-1:])


def scenario_convergence(b, ref):
    residuals = [np.uint32(s[1]).view(np.float32) for s in ref["states"]]
    low, high = float(residuals[STOP_AT - 1]), float(residuals[STOP_AT - 2])
    assert low < high, (low, high)
    tol = float(np.float32((low + high) / 2))
    assert low < tol <= high
    old_vectors, old_states = b.run(b.old_step, tol)
    old_final = b.both()
    assert old_states[-1][0] == STOP_AT and old_states[-1][2] == 1, old_states
    new_vectors, new_states = b.run(b.new_step, tol)
    new_final = b.both()
    assert new_states == old_states and new_states[-1][0] == STOP_AT, (new_states, old_states)
    same_vectors(new_vectors, old_vectors, "vectors seen after every enqueued step")
    same_vectors(new_final, old_final, "both rank vectors at the end")
    # the steps past STOP_AT were no-ops: the two vectors are what steps STOP_AT - 1 and STOP_AT wrote
    assert STOP_AT % 2 == 0                      # step k (0-based) writes r[(k + 1) & 1]: the last one wrote r[0]
    same_vectors(new_final, [ref["vectors"][STOP_AT - 1], ref["vectors"][STOP_AT - 2]],
                 "vectors of the last two committed steps")


def scenario_flush_paths(b, ref, torch):
    lead = 3

    def start(step):
        b.pr.reset()
        for k in range(lead):
            step(k, 0.0)

    def follow(action):
        """state and vectors after `lead` steps in either form followed by `action`: must not depend on the form"""
        seen = []
        for step in (b.old_step, b.new_step):
            start(step)
            extra = action()
            seen.append((b.status(), b.both(), extra))
        (s0, v0, e0), (s1, v1, e1) = seen
        assert s0 == s1 and e0 == e1, (action.__name__, s0, s1, e0, e1)
        same_vectors(v1, v0, action.__name__)
        return s1

    def status():
        return None
    assert follow(status) == ref["states"][lead - 1]

    def reset_then_two_steps():
        b.pr.reset()
        fresh = b.status()
        assert fresh[0] == 0 and fresh[2] == 0 and fresh[3] == 0, fresh
        b.old_step(0, 0.0)
        b.old_step(1, 0.0)
        return fresh
    assert follow(reset_then_two_steps) == ref["states"][1]

    def expand_then_step():
        b.eng.expand(b.pr.r[lead & 1], N)                     # every column final: all of phase 1 runs now
        b.old_step(lead, 0.0)
    assert follow(expand_then_step) == ref["states"][lead]

    def plain_step():
        b.old_step(lead, 0.0)
    assert follow(plain_step) == ref["states"][lead]

    side = torch.cuda.Stream()

    def step_on_a_second_stream():
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            b.new_step(lead, 0.0)
            after = b.status()                                # on the side stream
        torch.cuda.synchronize()
        return after
    assert follow(step_on_a_second_stream) == ref["states"][lead]

    # every path above left the shard usable: three more deferred steps agree with the reference run
    for k in range(lead + 1, lead + 4):
        b.new_step(k, 0.0)
    assert b.status() == ref["states"][lead + 3]


def scenario_destroy(spmv, prd, torch, rp, ci, va, fold, ref):
    b = Bench(spmv, prd, torch, rp, ci, va, fold)
    b.pr.reset()
    for k in range(3):
        b.new_step(k, 0.0)
    vectors = [b.bits(0), b.bits(1)]
    b.eng.close()                                             # destroys the shard with the commit of step 2 pending
    torch.cuda.synchronize()
    assert spmv.lib().spmv_c_device_synchronize() == 0
    got = [v.cpu().numpy().view(np.uint32) for v in vectors]
    same_vectors(got, [ref["vectors"][1], ref["vectors"][2]], "vectors when the shard is destroyed")
    b.pr.close()


def scenario_graph(b, ref, torch):
    from ctypes import POINTER, cast
    b.pr.reset()
    b.new_step(0, 0.0)                                        # warm-up pair outside the capture
    b.new_step(1, 0.0)
    assert b.status()[0] == 2                                 # ... and nothing pending when the capture begins
    b.pr.reset()
    torch.cuda.synchronize()
    mirror = torch.zeros(6, dtype=torch.int32).pin_memory()   # spmv_c_pr_status, filled by every replay
    out = cast(mirror.data_ptr(), POINTER(b.spmv.PrStatus))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.new_step(0, 0.0)
        b.new_step(1, 0.0)
        assert b.lib.spmv_c_pr_status_get(b.eng._shard, out, b._stream()) == 0
    b.pr.reset()
    for replay in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert status_tuple(out.contents) == ref["states"][2 * replay + 1], (replay, status_tuple(out.contents))
    assert b.status() == ref["states"][5]
    same_vectors(b.both(), [ref["vectors"][5], ref["vectors"][4]], "after three replays of two steps")


def worker_engine():
    import torch
    spmv = importlib.import_module("gpu-spmv_amd")
    prd = importlib.import_module("gpu-spmv_amd.pagerank_dist")
    spmv.require_gpu()
    outcome = {}

    def attempt(name, fn, *args):
        try:
            fn(*args)
            outcome[name] = "ok"
        except Exception as exc:                # noqa: BLE001 - reported to the test that owns the scenario
            import traceback
            outcome[name] = "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))[-2500:]

    for name, rp, ci, va, fold in matrices(spmv):
        b = Bench(spmv, prd, torch, rp, ci, va, fold)
        if name == "long_rows":
            assert b.info["long_rows"] == 3, b.info
        vectors, states = b.run(b.old_step, 0.0, status_each=True)      # the reference, computed once
        ref = {"vectors": vectors, "states": states}
        attempt(name + ":bit_equality", scenario_bit_equality, b, ref)
        attempt(name + ":convergence", scenario_convergence, b, ref)
        attempt(name + ":flush_paths", scenario_flush_paths, b, ref, torch)
        attempt(name + ":graph", scenario_graph, b, ref, torch)
        b.close()
        attempt(name + ":destroy", scenario_destroy, spmv, prd, torch, rp, ci, va, fold, ref)
    print("DEFERRED_COMMIT " + json.dumps(outcome), flush=True)


def switch_graph(spmv):
    """Slowly converging: node i is linked from 12 of the 2000 nodes in front of it only (the first nodes from
    fewer, the last node links nowhere: dangling), so rank travels down the line — 28 steps to 1e-6 where the
    uniform random graph of this size takes 6."""
    window = 2000
    offsets = spmv.synth.uniform_csr(94, 0, SWITCH_N, window, SWITCH_K)[1].reshape(SWITCH_N, SWITCH_K).astype(np.int64) + 1
    cols = np.arange(SWITCH_N, dtype=np.int64)[:, None] - offsets
    keep = cols >= 0
    cols = np.sort(np.where(keep, cols, SWITCH_N), axis=1)
    ci = cols[cols < SWITCH_N].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    assert ci.size >= 1 << 20
    return rp, ci, spmv.synth.column_stochastic_values(ci, SWITCH_N)


def worker_pagerank():
    """pagerank() on the switch graph in this process's environment -> iterations, flags, plan, error against the oracle"""
    spmv = importlib.import_module("gpu-spmv_amd")
    oracle = importlib.import_module("oracle")
    spmv.require_gpu()
    rp, ci, va = switch_graph(spmv)
    A = spmv.csr_from_arrays(SWITCH_N, SWITCH_N, rp, ci, va)
    assert spmv.csr_to_gpu(A) == 0
    r = spmv.pagerank(A, spmv.PageRankConfig(0.85, 1e-6, 100))
    planned = bool(spmv.csr_has_tiled_plan(A))
    # the oracle at the SAME number of steps (tolerance 0), as assert_parity of tests/test_gpu_pagerank.py does
    want, iters, _, _ = oracle.pagerank(rp, ci, va, num_cols=SWITCH_N, damping=0.85, tolerance=0.0,
                                        max_iterations=int(r.iterations), wide_sums=True)
    _, oracle_iters, _, oracle_conv = oracle.pagerank(rp, ci, va, num_cols=SWITCH_N, damping=0.85, tolerance=1e-6,
                                                      max_iterations=100, wide_sums=True)
    worst = float(np.max(np.abs(np.asarray(r.ranks, np.float64) - want) / want))
    spmv.csr_destroy(A)
    print("DEFERRED_COMMIT " + json.dumps({"iterations": int(r.iterations), "converged": bool(r.converged),
                                           "residual": float(r.final_residual), "planned": planned, "worst_rel": worst,
                                           "oracle_iterations": int(oracle_iters), "oracle_converged": bool(oracle_conv)}),
          flush=True)


# -------------------------------------------------------------------------------------------- test side ----
def run_worker(mode, **env):
    full = dict(os.environ, **env)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True,
                         timeout=600, env=full)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("DEFERRED_COMMIT ")]
    assert len(lines) == 1, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(lines[0][len("DEFERRED_COMMIT "):])


@pytest.fixture(scope="module")
def outcome(gpu):
    return run_worker("engine", SPMV_DEBUG="min_cols=1,min_nnz=1,strip=4096,tile=1024")


MATRICES = ("uniform", "long_rows")


@pytest.mark.parametrize("matrix", MATRICES)
def test_step_commit_equals_the_three_launch_form_bit_for_bit(outcome, matrix):
    """12 steps from the same start: the vector every step wrote and the status after every step (iterations,
    residual bits, flags) are equal — with a status call (a flush) after every step, and with one at the end only."""
    assert outcome[matrix + ":bit_equality"] == "ok", outcome[matrix + ":bit_equality"]


@pytest.mark.parametrize("matrix", MATRICES)
def test_steps_enqueued_past_convergence_are_no_ops(outcome, matrix):
    """A tolerance between the residuals of steps 5 and 6 stops the run at step 6 of 12 enqueued: iterations == 6,
    converged, and both vectors equal the three-launch form's bit for bit."""
    assert outcome[matrix + ":convergence"] == "ok", outcome[matrix + ":convergence"]


@pytest.mark.parametrize("matrix", MATRICES)
def test_every_flush_path_gives_the_state_of_the_three_launch_form(outcome, matrix):
    """step_commit x 3, then: status; reset (iterations == 0) and two more steps; expand of all columns and a step;
    a plain step + reduce_commit; a step_commit on a second stream.  Same status and vectors as after three steps of
    the old form followed by the same calls."""
    assert outcome[matrix + ":flush_paths"] == "ok", outcome[matrix + ":flush_paths"]


@pytest.mark.parametrize("matrix", MATRICES)
def test_shard_destroyed_with_a_commit_pending(outcome, matrix):
    assert outcome[matrix + ":destroy"] == "ok", outcome[matrix + ":destroy"]


@pytest.mark.parametrize("matrix", MATRICES)
def test_two_captured_steps_and_a_status_flush_replay_like_the_eager_loop(outcome, matrix):
    """hipGraph of step_commit (A -> B), step_commit (B -> A) and spmv_c_pr_status_get into pinned memory, replayed
    three times: the status every replay leaves and the vectors at the end equal the eager three-launch run's."""
    assert outcome[matrix + ":graph"] == "ok", outcome[matrix + ":graph"]


def test_pagerank_switching_engines_mid_run_counts_the_same_iterations(gpu):
    """pagerank() starts on the direct kernel (commit at once) and moves to the tiled engine after two steps
    (commits deferred from then on, the state mirror one step behind): every rank within 1e-5 of the oracle at the
    same number of steps, and that number is the one a run that never leaves the direct kernel (SPMV_TILED=0) counts."""
    switched = run_worker("pagerank", SPMV_DEBUG="pr_plan_after=2")
    direct = run_worker("pagerank", SPMV_TILED="0")
    print("switched:", switched, "direct:", direct)
    assert switched["planned"] and not direct["planned"]
    assert switched["worst_rel"] <= 1e-5 and direct["worst_rel"] <= 1e-5
    assert switched["converged"] and switched["converged"] == switched["oracle_converged"]
    assert abs(switched["iterations"] - switched["oracle_iterations"]) <= 1
    assert 2 < switched["iterations"] < 100                  # the switch happened mid-run
    assert switched["iterations"] == direct["iterations"]
    assert switched["converged"] == direct["converged"]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"engine": worker_engine, "pagerank": worker_pagerank}[sys.argv[1]]()
