"""Phase 2 of the tiled engine reads its row deltas from the pass-ordered copy the builder lays out (pass_word,
csrc/tiled_layout.h): one aligned 256-byte block per pass, four skip markers on the lanes past the pass's end.

Exact integer data, int64 reference, bit equality, as in tests/test_gpu_tiled_geometry.py.  The matrices are
tiled_model.pass_matrix (R = 64 and R = 9984, value stream and folded values): seven tiles, one per corner of the
pass stream — cells of exactly four slots, passes of three segments, a wavefront of more than 64 passes (a second
descriptor window), empty runs between full ones, skip markers opening a segment (R = 9984), a last pass of one group
(63 pad lanes) and long rows.  tests/test_tiled_model.py proves those claims on the host; here the model itself is
held to the device's plan first: its slot, item, long-row and pass counts must be the ones csr_tiled_info reports
(the passes through plan_bytes, which counts 32 + 256 bytes for each)."""
import importlib

import numpy as np
import pytest

import exact_data as ed
import tiled_model as tm

pytestmark = pytest.mark.gpu

sweep = importlib.import_module("test_gpu_lane_sweep")
assert_bits, Device = sweep.assert_bits, sweep.Device
VECTOR, MERGE = 1, 2


def assert_model(gpu, A, lay, W, R, cols, fold, what):
    info = gpu.csr_tiled_info(A)
    assert info is not None, what
    assert (info["strip_cols"], info["tile_rows"], info["num_strips"], info["num_tiles"], info["values_folded"]) == \
        (W, R, lay["S"], lay["T"], fold), (what, info)
    assert info["slots_in_cells"] == lay["slots"] and info["long_rows"] == lay["long_rows"], (what, info)
    assert gpu.csr_tiled_items(A) == len(lay["items"]), what
    assert info["plan_bytes"] == tm.plan_bytes(lay, cols, fold), (what, info, tm.num_passes(lay))
    return info


@pytest.mark.parametrize("R,fold", tm.PASS_CASES)
def test_every_corner_of_the_pass_stream(gpu, monkeypatch, R, fold):
    rows, cols, rp, ci, va, x, lay = tm.pass_matrix(R, fold)
    want = ed.exact_reference(rp, ci, va, x)
    monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(tm.PASS_W, R))
    monkeypatch.setenv("SPMV_TILED_FOLD", "1" if fold else "0")
    D = Device(gpu, rp, ci, va, cols)
    try:
        gpu.csr_invalidate_gpu_cache(D.A)
        for kernel in (VECTOR, MERGE):
            for call in (0, 1):                          # the later calls meet the first one's product scratch
                assert_bits(rp, D.run(x, kernel, use_texture=True), want, ("pass stream", R, fold, kernel, call))
        info = assert_model(gpu, D.A, lay, tm.PASS_W, R, cols, fold, ("pass stream", R, fold))
        # the pass-ordered copy replaces the slot-ordered bytes: what it adds is the unused tail of the passes
        print("R", R, "fold", fold, "slots", lay["slots"], "passes", tm.num_passes(lay), "plan_bytes", info["plan_bytes"])
    finally:
        D.close()


@pytest.mark.parametrize("R,fold", [(64, False), (9984, False)], ids=["general", "marker_heavy"])
def test_builder_forms_give_one_pass_stream(gpu, monkeypatch, R, fold):
    """place=scattered against the staged placing pass, rank=plain against stable binning: the checksum of the
    pass-ordered row deltas (third of the four) is a function of the matrix alone, like the other three."""
    rows, cols, rp, ci, va, x, lay = tm.pass_matrix(R, fold)
    assert R == 64 or int((lay["drow"] == tm.SKIP).sum()) > 100
    want = ed.exact_reference(rp, ci, va, x)
    monkeypatch.setenv("SPMV_TILED_FOLD", "0")
    D = Device(gpu, rp, ci, va, cols)
    try:
        sums = {}
        for form in ("", "place=scattered", "rank=plain", "place=scattered,rank=plain"):
            monkeypatch.setenv("SPMV_DEBUG", ed.tiled_debug(tm.PASS_W, R, form))
            gpu.csr_invalidate_gpu_cache(D.A)
            assert_bits(rp, D.run(x, VECTOR, use_texture=True), want, ("forms", R, form))
            assert_model(gpu, D.A, lay, tm.PASS_W, R, cols, fold, ("forms", R, form))
            sums[form] = gpu.csr_tiled_checksum(D.A)
            assert sums[form] is not None and sums[form][2] != 0 and sums[form] == sums[""], (R, form, sums)
    finally:
        D.close()
