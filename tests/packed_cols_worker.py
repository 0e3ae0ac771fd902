"""Worker of tests/test_gpu_packed_cols.py: the tiled engine's phase 1 on plans whose local columns are packed to 14
bits in 448-byte blocks (csrc/tiled_layout.h), against an int64 / integer evaluation in numpy AND against the same
call on a plan built under SPMV_DEBUG=cols=u16 (the unpacked array), bit for bit.

One process runs every group and prints one "GROUP name ok ..." line per group, or "GROUP name FAILED ..." with what
differed: the test module runs this once and asserts on the lines.  SPMV_DEBUG is read at every plan build, so each
case sets it and builds a fresh matrix handle.  Exact data throughout (tests/exact_data.py): small integers, every x_j
distinct wherever a wrong column has to show, so NO tolerance anywhere.

That a plan really is packed (or really is not) is read off csr_tiled_info's col_bytes: a packed plan holds
448 * ceil(slots / 256) + 8 bytes of columns where the u16 plan holds 2 * slots.  plan_bytes counts two bytes a slot
for either form (tests/tiled_model.py holds it to that), so it must not differ between the two."""
import importlib
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
spmv = importlib.import_module("gpu-spmv_amd")
import exact_data as ed  # noqa: E402

VECTOR, MERGE = 1, 2
BLOCK_SLOTS, BLOCK_BYTES, SLACK = 256, 448, 8


def packed_bytes(slots):
    return -(-slots // BLOCK_SLOTS) * BLOCK_BYTES + SLACK


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_spmv(rows, cols, rp, ci, va, x, debug, fold):
    """y of VECTOR_CSR and MERGE_PATH with use_texture (the second call meets the first one's scratch) on a plan
    built under `debug`; the plan's info, item count and checksums."""
    os.environ["SPMV_DEBUG"] = debug
    os.environ["SPMV_TILED_FOLD"] = "1" if fold else "0"
    A = spmv.csr_from_arrays(rows, cols, rp, ci, va)
    assert spmv.csr_to_gpu(A) == 0
    d_x, d_y = spmv.CudaBuffer(cols), spmv.CudaBuffer(rows)
    d_x.copyFromHost(x, cols)
    try:
        ys = []
        for kernel in (VECTOR, MERGE):
            d_y.copyFromHost(np.full(rows, np.float32(-12345.0)), rows)
            assert spmv.spmv_csr(A, d_x, d_y, spmv.SpMVConfig(kernel_type=kernel, use_texture=True), cols).error_code == 0
            ys.append(d_y.copyToHost(rows))
        info = spmv.csr_tiled_info(A)
        assert info is not None, "no plan under " + debug
        info = dict(info, items=spmv.csr_tiled_items(A), checksum=spmv.csr_tiled_checksum(A))
        assert info["values_folded"] == fold, info
        return ys, info
    finally:
        spmv.csr_destroy(A)
        d_x.release()
        d_y.release()


def both_forms(what, rows, cols, rp, ci, va, x, W, R, fold, extra="item=1024"):
    """The case on the packed plan and on the cols=u16 plan: equal bits, equal to the integer reference; equal
    checksums; the column bytes each form claims.  Returns the packed plan's info."""
    ed.check_exact(rp, ci, va, x)
    want = ed.exact_reference(rp, ci, va, x)
    debug = ed.tiled_debug(W, R, extra)
    ys_p, info_p = run_spmv(rows, cols, rp, ci, va, x, debug, fold)
    ys_u, info_u = run_spmv(rows, cols, rp, ci, va, x, debug + ",cols=u16", fold)
    for name, ys in (("packed", ys_p), ("u16", ys_u)):
        for call, y in enumerate(ys):
            bad = np.flatnonzero(bits(y) != bits(want))
            assert bad.size == 0, (what, name, call, bad.size, [(int(r), float(y[r]), float(want[r])) for r in bad[:6]])
    for a, b in zip(ys_p, ys_u):
        assert np.array_equal(bits(a), bits(b)), what
    assert info_p["strip_cols"] == W and info_u["strip_cols"] == W, (what, info_p)
    slots = info_p["slots_in_cells"]
    assert slots == info_u["slots_in_cells"] and info_p["items"] == info_u["items"], (what, info_p, info_u)
    assert info_u["col_bytes"] == 2 * slots, (what, info_u)
    assert info_p["col_bytes"] == (packed_bytes(slots) if W <= 16384 and slots > 0 else 2 * slots), (what, info_p)
    assert info_u["plan_bytes"] == info_p["plan_bytes"], (what, info_u["plan_bytes"], info_p["plan_bytes"])
    assert info_p["checksum"] is not None and info_p["checksum"] == info_u["checksum"], (what, info_p["checksum"], info_u["checksum"])
    return info_p


def distinct_x(rng, cols):
    """Every x_j another integer, in random order: a product read at a wrong column is a wrong product."""
    return rng.permutation(np.arange(cols, dtype=np.int64) - cols // 2).astype(np.float32)


def values_for(rng, ci, cols, fold, vmax):
    if fold:
        weight = (rng.integers(1, vmax + 1, size=cols) * rng.choice([-1, 1], size=cols)).astype(np.float32)
        return weight[ci]
    return (rng.integers(1, vmax + 1, size=ci.size) * rng.choice([-1, 1], size=ci.size)).astype(np.float32)


def csr_of(rows, cols, rr, cc):
    keys = np.unique(np.asarray(rr, np.int64) * cols + np.asarray(cc, np.int64))
    rr, ci = keys // cols, (keys % cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=rows))]).astype(np.int32)
    return rp, ci


# ------------------------------------------------------------------------------------------ strip widths, column extremes
def extreme_columns(W, cols):
    """Local columns 0, 255, 256 and the last one a strip has (16383 where it has that many) of the first, a middle
    and the last, partial, strip."""
    strips = -(-cols // W)
    out = []
    for s in (0, strips // 2, strips - 1):
        width = min(W, cols - s * W)
        out.append([s * W + c for c in (0, 255, 256, min(16383, width - 1), width - 1)])
    return out


def strip_width_case(W, fold):
    """2000 rows over three and a bit strips, ~12 entries per row, and three rows that hold nothing but the extreme
    local columns of one strip each."""
    rng = np.random.default_rng(W + int(fold))
    rows, cols = 2000, 3 * W + 1000
    rr = np.repeat(np.arange(rows), 12)
    cc = rng.integers(0, cols, size=rr.size)
    special = (7, rows // 2, rows - 1)
    keep = ~np.isin(rr, special)
    rr, cc = list(rr[keep]), list(cc[keep])
    for row, columns in zip(special, extreme_columns(W, cols)):
        rr += [row] * len(columns)
        cc += columns
    rp, ci = csr_of(rows, cols, rr, cc)
    va = values_for(rng, ci, cols, fold, 4)
    x = distinct_x(rng, cols)
    for row, columns in zip(special, extreme_columns(W, cols)):       # the extreme rows hold exactly those columns
        assert sorted(set(columns)) == list(ci[rp[row]:rp[row + 1]])
    info = both_forms(("strip", W, fold), rows, cols, rp, ci, va, x, W, 1024, fold)
    assert info["num_strips"] == 4 and info["items"] >= 4, info
    return info["slots_in_cells"]


# ------------------------------------------------------------------------------------------ block positions
POSITION_W, POSITION_R = 4096, 4096
# slots per strip (one tile: a strip is one cell).  64 strips of 260 = 256 + 4 slots: strip s begins at slot 260 s, at
# group s of its block, so begins and ends fall on every one of the 64 four-slot positions and strip 63 begins in a
# block's LAST group; then two strips that item=1024 cuts into three and two items, and a last strip that ends the array
# on a block boundary: the last lane of the final block is in use, and its 4-byte read of the high bits runs into the
# slack behind the array.
POSITION_CELLS = [260] * 64 + [2052, 1028, 248]


def block_position_case(fold):
    rng = np.random.default_rng(77 + int(fold))
    rows, cols = POSITION_R, len(POSITION_CELLS) * POSITION_W
    rr, cc = [], []
    for s, n in enumerate(POSITION_CELLS):
        i = np.arange(n)
        rr.append(i)                                         # rows 0 .. n - 1 (n <= rows): every delta 0 or 1, no markers
        cc.append(s * POSITION_W + (i * 61 + 3 * s) % POSITION_W)
    rp, ci = csr_of(rows, cols, np.concatenate(rr), np.concatenate(cc))
    assert ci.size == sum(POSITION_CELLS)
    va = values_for(rng, ci, cols, fold, 1)
    x = distinct_x(rng, cols)
    info = both_forms(("positions", fold), rows, cols, rp, ci, va, x, POSITION_W, POSITION_R, fold)
    begins = np.concatenate([[0], np.cumsum(POSITION_CELLS)])
    assert info["slots_in_cells"] == begins[-1] and begins[-1] % BLOCK_SLOTS == 0, info
    assert sorted(set((begins[:64] % BLOCK_SLOTS) // 4)) == list(range(64)) and begins[63] % BLOCK_SLOTS == 252
    assert info["num_strips"] == len(POSITION_CELLS) and info["num_tiles"] == 1 and info["long_rows"] == 0, info
    assert info["items"] == 64 + 3 + 2 + 1, info
    return info["slots_in_cells"]


# ------------------------------------------------------------------------------------------ a plan of less than one block
def tiny_case(fold):
    rng = np.random.default_rng(5 + int(fold))
    rows, cols = 10, 5000
    rr = np.repeat(np.arange(rows), 3)
    cc = rng.integers(0, cols, size=rr.size)
    cc[:4] = (0, 255, 256, 4095)
    rp, ci = csr_of(rows, cols, rr, cc)
    va = values_for(rng, ci, cols, fold, 8)
    x = distinct_x(rng, cols)
    info = both_forms(("tiny", fold), rows, cols, rp, ci, va, x, 4096, 64, fold)
    assert 0 < info["slots_in_cells"] < BLOCK_SLOTS, info
    return info["slots_in_cells"]


# ------------------------------------------------------------------------------------------ checksums
def checksum_matrices():
    rng = np.random.default_rng(11)
    rows, cols = 20000, 40000
    uniform = (np.repeat(np.arange(rows), 8), rng.integers(0, cols, size=rows * 8), 1024)
    lens = np.minimum((rng.pareto(1.2, size=rows) * 3).astype(np.int64) + 1, 3000)
    power = (np.repeat(np.arange(rows), lens), rng.integers(0, cols, size=int(lens.sum())), 1024)
    # every 700th of ten times as many rows, three entries each: an entry drags at least two skip markers along
    sparse_rows = np.arange(0, 10 * rows, 700)
    marker = (np.repeat(sparse_rows, 3), rng.integers(0, cols, size=sparse_rows.size * 3), 9984)
    return rows, cols, {"uniform": uniform, "power_law": power, "marker_heavy": marker}


def checksum_case(name):
    rows, cols, cases = checksum_matrices()
    rr, cc, R = cases[name]
    rows = 10 * rows if name == "marker_heavy" else rows
    rp, ci = csr_of(rows, cols, rr, cc)
    rng = np.random.default_rng(12)
    va = values_for(rng, ci, cols, False, 2)
    x = rng.integers(-8, 9, size=cols).astype(np.float32)
    info = both_forms(("checksum", name), rows, cols, rp, ci, va, x, 8192, R, False, extra="")
    if name == "marker_heavy":
        assert info["slots_in_cells"] > 2 * info["entries_in_cells"], info       # markers outnumber the entries
    return info["checksum"][1]


# ------------------------------------------------------------------------------------------ PageRank
PAGERANK_CASES = ("n16_4096x64_sources_fold", "n16_8192x1024_sources_stream", "n16_16384x9984_dangling_stream")


def pagerank_case(name):
    n, W, R, _, fold, _, _ = ed.DYADIC_TILED[name]
    _, rp, ci, va, steps, want, _ = ed.dyadic_case(name)
    assert steps >= 1
    os.environ["SPMV_TILED_FOLD"] = "1" if fold else "0"
    got = {}
    for form in ("", ",cols=u16"):
        os.environ["SPMV_DEBUG"] = ed.tiled_debug(W, R, "pr_plan_after=0") + form
        A = spmv.csr_from_arrays(n, n, rp, ci, va)
        assert spmv.csr_to_gpu(A) == 0
        try:
            for call in (0, 1):
                r = spmv.pagerank(A, spmv.PageRankConfig(ed.DYADIC_DAMPING, 0.0, steps))
                assert r.iterations == steps and spmv.csr_has_tiled_plan(A), (name, form, r.iterations)
                bad = np.flatnonzero(bits(r.ranks) != bits(want))
                assert bad.size == 0, (name, form, call, bad.size, bad[:6])
            info = spmv.csr_tiled_info(A)
            assert info["strip_cols"] == W and info["values_folded"] == fold, info
            got[form] = (bits(r.ranks).copy(), np.float32(r.final_residual), info["col_bytes"], info["slots_in_cells"])
        finally:
            spmv.csr_destroy(A)
    assert np.array_equal(got[""][0], got[",cols=u16"][0]) and bits(got[""][1]) == bits(got[",cols=u16"][1]), name
    slots = got[""][3]
    assert (got[""][2], got[",cols=u16"][2]) == (packed_bytes(slots), 2 * slots), (name, got[""][2], got[",cols=u16"][2])
    return steps


def main():
    spmv.require_gpu()
    groups = []
    for W in (4096, 8192, 16384, 32768):
        for fold in (False, True):
            groups.append(("strip_%d_%s" % (W, "fold" if fold else "stream"), lambda W=W, fold=fold: strip_width_case(W, fold)))
    for fold in (False, True):
        groups.append(("positions_%s" % ("fold" if fold else "stream"), lambda fold=fold: block_position_case(fold)))
        groups.append(("tiny_%s" % ("fold" if fold else "stream"), lambda fold=fold: tiny_case(fold)))
    for name in ("uniform", "power_law", "marker_heavy"):
        groups.append(("checksum_" + name, lambda name=name: checksum_case(name)))
    for name in PAGERANK_CASES:
        groups.append(("pagerank_" + name, lambda name=name: pagerank_case(name)))
    failed = 0
    for name, run in groups:
        try:
            print("GROUP %s ok %s" % (name, run()), flush=True)
        except Exception:                                    # every group reports; the test module asserts on each line
            failed += 1
            print("GROUP %s FAILED %s" % (name, traceback.format_exc().replace("\n", " | ")[-1500:]), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
