"""What tests/tiled_model.py claims about its matrices, proved without a GPU: every corner of the phase-2 pass stream
(PASS_CASES) and of the phase-1 item origin (CHUNK_CASES) that the GPU tests name is reached by the layout the model
derives, and the host logic picks the forced shape."""
import numpy as np
import pytest

import exact_data as ed
import tiled_model as tm


@pytest.mark.parametrize("R,fold", tm.PASS_CASES)
def test_pass_matrix_reaches_every_corner_of_the_pass_stream(R, fold):
    rows, cols, rp, ci, va, x, lay = tm.pass_matrix(R, fold)
    assert (lay["S"], lay["T"]) == (tm.PASS_STRIPS, len(tm.PASS_TILES))
    assert int(np.diff(rp).max()) > ed.default_long_row(lay["S"])
    tm.pass_claims(R, lay)
    assert (lay["drow"] == tm.SKIP).sum() >= (40 if R > 700 else 1)
    assert tm.num_passes(lay) * tm.PASS_SLOTS >= lay["slots"]


@pytest.mark.parametrize("W,fold", tm.CHUNK_CASES)
def test_chunk_matrix_puts_item_begins_at_every_offset_of_a_chunk(W, fold):
    rows, cols, rp, ci, va, x, lay = tm.chunk_matrix(W, fold)
    assert (lay["S"], lay["T"]) == (len(tm.CHUNK_STRIP_SLOTS), tm.CHUNK_TILES)
    tm.chunk_claims(lay)


def test_the_model_counts_skip_markers_like_the_builder():
    """One cell, rows 0, 254, 255, 510, 1000 of a 9984-row tile: gaps 0, 254, 1, 255, 490 -> 0, 0, 0, 1, 1 markers."""
    rr = np.array([0, 254, 255, 510, 1000])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=9984))]).astype(np.int32)
    lay = tm.layout(rp, np.zeros(5, np.int32), 4096, 4096, 9984, 64, 4096)
    assert lay["slots"] == 8 and list(lay["drow"]) == [0, 254, 1, 255, 0, 255, 235, 255]
