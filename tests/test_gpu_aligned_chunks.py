"""Phase 1 of the tiled engine walks a work item from the 16-slot boundary at or below its first slot, so that every
full store instruction of a wavefront writes whole 64-byte sectors of products; the groups in front of the item are
masked like those behind it (expand_slots, csrc/tiled.hip).

Exact integer data, int64 reference, bit equality.  tiled_model.chunk_matrix at item=1024, for each of the four strip
widths, value stream and folded values (all eight tiled_expand_kernel instantiations): items that begin 0, 4, 8 and 12
slots past a boundary, an item shorter than 16 slots that begins at 12, items of exactly 16 k slots from an aligned and
from an unaligned begin, strips holding a single cell, and strips cut into several items inside a cell.
tests/test_tiled_model.py proves those claims on the host; the model's slot and item counts must be the plan's."""
import importlib

import pytest

import exact_data as ed
import tiled_model as tm

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
pass_tests = importlib.import_module("test_gpu_pass_stream")
assert_bits, Device = sweep.assert_bits, sweep.Device
VECTOR, MERGE = 1, 2


@pytest.mark.parametrize("W,fold", tm.CHUNK_CASES)
def test_item_begins_at_every_offset_of_a_chunk(gpu, monkeypatch, W, fold):
    rows, cols, rp, ci, va, x, lay = tm.chunk_matrix(W, fold)
    want = ed.exact_reference(rp, ci, va, x)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(W, tm.CHUNK_R, "item=%d" % tm.CHUNK_ITEM))
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if fold else "0")
    D = Device(gpu, rp, ci, va, cols)
    try:
        gpu.csr_invalidate_gpu_cache(D.A)
        for kernel in (VECTOR, MERGE):
            for call in (0, 1):
                assert_bits(rp, D.run(x, kernel, use_texture=True), want, ("chunks", W, fold, kernel, call))
        pass_tests.assert_model(gpu, D.A, lay, W, tm.CHUNK_R, cols, fold, ("chunks", W, fold))
    finally:
        D.close()
