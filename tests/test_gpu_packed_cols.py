"""Phase 1 of the tiled engine on plans whose local columns are packed to 14 bits (csrc/tiled_layout.h: blocks of 256
slots in 448 bytes, a low plane of bytes and a field of 6-bit high parts), held to bit equality with an integer
evaluation in numpy and with the same call on a plan built under SPMV_DEBUG=cols=u16, which keeps the u16 array.

tests/packed_cols_worker.py runs every group in one process (one import of the library, one GPU context) and prints a
line per group; the worker runs once per session and each test below asserts on its group's line:

  strip_W_stream / strip_W_fold   W = 4096, 8192, 16384 packed, 32768 kept as u16; value stream and folded values;
                                  entries at local columns 0, 255, 256 and the last of the first, a middle and the
                                  last, partial, strip; every x_j distinct
  positions_*                     item begins and ends on every 4-slot position of a block, an item that begins in a
                                  block's last group, a last item that ends with the array's final block (the 4-byte
                                  read of the last lane's high bits runs into the slack behind the array)
  tiny_*                          a plan of fewer than 256 slots
  checksum_*                      tiled_checksum with and without cols=u16 on a uniform, a power-law and a
                                  marker-heavy matrix (every group compares the checksums; these three are about them)
  pagerank_*                      the PageRank vector and residual of exact_data's dyadic graphs at W = 4096, 8192, 16384"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

GROUPS = (["strip_%d_%s" % (W, f) for W in (4096, 8192, 16384, 32768) for f in ("stream", "fold")] +
          ["positions_stream", "positions_fold", "tiny_stream", "tiny_fold"] +
          ["checksum_uniform", "checksum_power_law", "checksum_marker_heavy"] +
          ["pagerank_n16_4096x64_sources_fold", "pagerank_n16_8192x1024_sources_stream",
           "pagerank_n16_16384x9984_dangling_stream"])


@pytest.fixture(scope="module")
def worker_lines(gpu):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "packed_cols_worker.py")],
                         capture_output=True, text=True, timeout=600, env=dict(os.environ))
    lines = {}
    for line in out.stdout.splitlines():
        if line.startswith("GROUP "):
            lines[line.split()[1]] = line
    return out, lines


@pytest.mark.parametrize("group", GROUPS)
def test_packed_columns(worker_lines, group):
    out, lines = worker_lines
    assert group in lines, (group, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert lines[group].startswith("GROUP %s ok" % group), lines[group]


def test_worker_ran_every_group_and_nothing_else(worker_lines):
    out, lines = worker_lines
    assert sorted(lines) == sorted(GROUPS), (sorted(lines), out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
