"""bench.py end to end on the GPU box (small matrix): stdout is exactly one JSON line with the contract's keys, a plain
run measures only its headline and writes what its last step computed (--dump-outputs), and under --full the
line survives a failing extra and a failing exchange trial (protocol of the reference's
include/spmv/benchmark.h:34-40: warm-up, timed iterations, one record out)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--rows", "400000", "--steps", "3", "--warmup", "1"]


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def one_line(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_one_line_with_the_contract_keys(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--no-extras"] + SMALL,
                         capture_output=True, text=True, timeout=900)
    line = one_line(out)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["steps"] == 3 and line["n_gpus"] == 1 and line["value"] > 0
    roof = line["roofline"]
    assert roof["bound"] == "hbm" and 0 < roof["frac"] < 1 and roof["peak"] == 8000.0
    assert "incomplete" not in line and "provisional" not in line


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(gpu, oracle, tmp_path):
    """No --full: the steps it was asked for and nothing after them (no roofline launches, no extras); --dump-outputs
    holds the rank vector after the W + K steps, which is W + K PageRank iterations of the oracle on the same matrix."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(tmp_path / "out")] + SMALL,
                         capture_output=True, text=True, timeout=900)
    line = one_line(out)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert "roofline" not in line and line["cpu_baseline"] is None and "extras_done" not in line
    assert sorted(os.listdir(tmp_path / "out")) == ["ranks.npy", "residual.npy"]
    ranks, residual = np.load(tmp_path / "out" / "ranks.npy"), np.load(tmp_path / "out" / "residual.npy")
    assert ranks.dtype == np.float32 and residual.dtype == np.float64 and residual.shape == (1,)
    n = line["config"]["rows"]
    rp, ci, _ = gpu.synth.uniform_csr(42, 0, n, n, line["config"]["avg_nnz_per_row"])
    va = gpu.synth.column_stochastic_values(ci, n)
    want, *_ = oracle.pagerank(rp, ci, va, num_cols=n, tolerance=0.0, max_iterations=4, wide_sums=True)
    got = ranks.astype(np.float64)
    assert ranks.shape == (n,) and np.isfinite(residual).all() and residual[0] >= 0
    worst = float(np.max(np.abs(got / got.sum() - want) / np.abs(want)))
    assert worst <= 1e-5, worst


@pytest.mark.gpu
def test_an_extra_that_kills_the_process_costs_the_extra_only(gpu):
    env = dict(os.environ, SPMV_BENCH_FAIL_IN="cpu_baseline:abort")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + SMALL, capture_output=True,
                         text=True, timeout=900, env=env)
    line = one_line(out)
    assert line["value"] > 0 and "incomplete" in line and line["roofline"]["frac"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["raise", "abort"])
def test_two_ranks_a_failing_exchange_trial_still_leaves_the_line(gpu, how):
    """Two ranks sharing the one GPU over gloo (a rehearsal of the N > 1 code path; its number means nothing)."""
    env = dict(os.environ, SPMV_BENCH_BACKEND="gloo", SPMV_PR_OVERLAP="2", SPMV_BENCH_FAIL_IN="trial:" + how)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
                          os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full"] + SMALL,
                         capture_output=True, text=True, timeout=1200, env=env)
    line = one_line(out)
    assert line["n_gpus"] == 2 and line["config"]["exchange"] == "gather" and line["value"] > 0


@pytest.mark.gpu
def test_plain_launch_with_two_gpus_starts_its_own_launcher(gpu):
    """`python bench.py --gpus 2` the way the driver starts `--gpus 1` (no torch.distributed.run in front, no rank variables):
    the supervisor starts the launcher itself and exactly one line with n_gpus = 2 comes out."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["SPMV_BENCH_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-extras"] + SMALL,
                         capture_output=True, text=True, timeout=1200, env=env)
    line = one_line(out)
    assert line["n_gpus"] == 2 and line["config"]["exchange"] == "gather" and line["value"] > 0
    assert line["child_exit"] == "exit code 0" and "incomplete" not in line
    assert "starting torch.distributed.run" in out.stderr
