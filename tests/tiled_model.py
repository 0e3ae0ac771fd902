"""The tiled engine's plan layout on the host, for tests that must KNOW which corner of it a matrix reaches.

A plain module (not a test).  layout() restates what the builder writes (csrc/tiled_cells.hip, tiled_build.hip;
contract in csrc/tiled_layout.h): the slots of every cell (entries, 255-row skip markers, padding to four), the
row-delta byte of every slot, the phase-1 items and, per (tile, wavefront), the phase-2 passes with their segments.
tests/test_tiled_model.py proves the claims of the catalogue below without a GPU; the GPU tests hold the model itself
to the plan the device built (slot, item and pass counts from csr_tiled_info) before they rely on it.

The catalogue: PASS_CASES (tests/test_gpu_pass_stream.py) and CHUNK_CASES (tests/test_gpu_aligned_chunks.py)."""
import numpy as np

import exact_data as ed

SKIP = 255                    # kSkip
PASS_SLOTS, PASS_SEGS, WAVES = 256, 3, 16
LONG_CHUNK = 512


def layout(rp, ci, num_cols, W, R, long_limit, item_slots):
    """dict: S, T, cell_len [S, T] (padded slots), cell_off [S, T] (strip-major), drow (the row-delta byte of every
    slot), slots, long_rows, long_chunks, items [(strip, begin, end)], passes {(tile, wave): [[(begin, length), ...]]}."""
    rp = np.asarray(rp, np.int64)
    rows = rp.size - 1
    lens = np.diff(rp)
    S, T = -(-num_cols // W), -(-rows // R)
    long_rows = np.flatnonzero(lens > long_limit)
    rr = np.repeat(np.arange(rows, dtype=np.int64), lens)
    cc = np.asarray(ci, np.int64)
    keep = ~np.isin(rr, long_rows)
    rr, cc = rr[keep], cc[keep]
    cell = (cc // W) * T + rr // R
    order = np.lexsort((cc, rr, cell))                       # a cell's entries by (row, column)
    cell, local = cell[order], (rr % R)[order]
    first = np.ones(cell.size, bool)
    first[1:] = cell[1:] != cell[:-1]
    gap = local - np.where(first, 0, np.concatenate([[0], local[:-1]]))
    markers = gap // SKIP
    raw = np.bincount(cell, weights=1 + markers, minlength=S * T).astype(np.int64)
    cell_len = (raw + 3) // 4 * 4
    cell_off = np.concatenate([[0], np.cumsum(cell_len)])
    slots = int(cell_off[-1])
    drow = np.full(slots, SKIP, np.uint8)
    upto = np.cumsum(1 + markers)                            # slots used up to and including each entry ...
    start = np.concatenate([[0], upto])[np.flatnonzero(first)]
    upto_in_cell = upto - np.repeat(start, np.diff(np.concatenate([np.flatnonzero(first), [cell.size]])))
    drow[cell_off[cell] + upto_in_cell - 1] = gap % SKIP
    cell_len, cell_off = cell_len.reshape(S, T), cell_off[:-1].reshape(S, T)
    strip_begin = np.concatenate([cell_off[:, 0], [slots]])

    items = []                                               # make_items (tiled_build.hip)
    for s in range(S):
        begin, stop = int(strip_begin[s]), int(strip_begin[s + 1])
        parts = -(-(stop - begin) // item_slots)
        b = begin
        for part in range(1, parts + 1):
            nxt = stop if part == parts else (begin + (stop - begin) * part // parts) // 8 * 8
            nxt = max(nxt, b)
            if nxt == b and part != parts:
                continue
            items.append((s, b, nxt))
            b = nxt

    per_wave = -(-S // WAVES)
    assert per_wave <= 64, "the builder reads a wavefront's runs 64 at a time: not modelled beyond"
    passes = {}
    for t in range(T):                                       # pass_layout_kernel (tiled_cells.hip)
        for w in range(WAVES):
            lo, hi = min(S, w * per_wave), min(S, w * per_wave + per_wave)
            runs = [(int(cell_off[s, t]), int(cell_len[s, t])) for s in range(lo, hi)]
            mine, nxt, begin, length, off = [], 0, 0, 0, 0
            while True:
                segs, filled = [], 0
                for _ in range(PASS_SEGS):
                    while off >= length and nxt < len(runs):
                        begin, length = runs[nxt]
                        off, nxt = 0, nxt + 1
                    take = max(min(length - off, PASS_SLOTS - filled), 0)
                    if take:
                        segs.append((begin + off, take))
                    filled += take
                    off += take
                if not filled:
                    break
                mine.append(segs)
            if mine:
                passes[(t, w)] = mine
    chunks = int(sum(-(-int(lens[r]) // LONG_CHUNK) for r in long_rows))
    return dict(S=S, T=T, cell_len=cell_len, cell_off=cell_off, drow=drow, slots=slots, long_rows=long_rows.size,
                long_chunks=chunks, items=items, passes=passes)


def num_passes(lay):
    return sum(len(p) for p in lay["passes"].values())


def plan_bytes(lay, num_cols, fold):
    """build_plan's accounting (tiled_build.hip): products, local columns, values or column weights, cell table, pass
    descriptors + pass-ordered row deltas (32 + 256 bytes per pass), pass_first, items, long-row chunks."""
    S, T = lay["S"], lay["T"]
    return (lay["slots"] * (4 + 2 + (0 if fold else 4)) + S * T * 8 + num_passes(lay) * (32 + PASS_SLOTS)
            + 4 * (T * WAVES + 1) + (4 * num_cols if fold else 0) + 12 * len(lay["items"]) + 12 * lay["long_chunks"])


def _csr(rows, num_cols, rr, cc, fold, seed):
    """Distinct (row, column) pairs -> CSR with small integer values (one weight per column when folded) and x."""
    rng = np.random.default_rng(seed)
    keys = np.unique(np.asarray(rr, np.int64) * num_cols + np.asarray(cc, np.int64))
    rr, ci = keys // num_cols, (keys % num_cols).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=rows))]).astype(np.int32)
    if fold:
        weight = (rng.integers(1, 9, size=num_cols) * rng.choice([-1, 1], size=num_cols)).astype(np.float32)
        va = weight[ci]
    else:
        va = (rng.integers(1, 9, size=ci.size) * rng.choice([-1, 1], size=ci.size)).astype(np.float32)
    x = rng.integers(-64, 65, size=num_cols).astype(np.float32)
    ed.check_exact(rp, ci, va, x)
    return rp, ci, va, x


def _block(tile, R, strip, W, local_rows, per_row):
    """per_row entries in each of the tile's local rows `local_rows`, all inside one strip, distinct columns."""
    assert per_row <= 500
    local_rows = np.asarray(local_rows, np.int64)
    rr = np.repeat(tile * R + local_rows, per_row)
    cc = strip * W + np.tile(np.arange(per_row), local_rows.size) + np.repeat(local_rows % 5, per_row) * 500
    return rr, cc


# ------------------------------------------------------------------------------------------ phase 2: the pass stream
PASS_W, PASS_STRIPS = 4096, 48                 # three strips per wavefront
PASS_TILE_ROWS = (64, 9984)
PASS_CASES = [(R, fold) for R in PASS_TILE_ROWS for fold in (False, True)]
PASS_TILES = dict(four=0, three_segments=1, many_passes=2, empty_between=3, marker_first=4, one_group=5, long_rows=6)
_pass_cache = {}


def pass_matrix(R, fold):
    """(rows, cols, rp, ci, va, x, layout): seven tiles, each built for one corner of the pass stream (PASS_TILES).
      four            every cell holds exactly 4 slots (3 entries + padding, or 4 entries)
      three_segments  cells of 100 slots: a wavefront's 300 slots are a pass of 100 + 100 + 56 and one of 44
      many_passes     wavefront 0 owns more than 64 passes: a second descriptor window
      empty_between   strips 3 and 5 full, strip 4 empty (one wavefront); strips 9 and 11 likewise with one entry
      marker_first    R = 9984 only: cells whose first entry lies 300 and 700 rows into the tile, so the run (a segment)
                      starts with skip markers; the second such cell follows a 252-slot one, so that its markers open
                      segment 1 of a pass.  (At R = 64 no delta reaches 255 and padding never opens a segment: segments
                      start on multiples of four slots, padding fills the end of a group.)
      one_group       a wavefront of 256 + 4 slots: its last pass has one group, 63 pad lanes
      long_rows       two rows beyond the long-row limit, short rows beside them"""
    if (R, fold) in _pass_cache:
        return _pass_cache[(R, fold)]
    W, S = PASS_W, PASS_STRIPS
    rows, cols = len(PASS_TILES) * R, S * W
    limit = ed.default_long_row(S)
    parts = []
    t = PASS_TILES["four"]
    for s in range(S):
        parts.append(_block(t, R, s, W, np.arange(3 + s % 2) * 7 + s % 9, 1))
    t = PASS_TILES["three_segments"]
    for s in range(S):
        parts.append(_block(t, R, s, W, np.arange(50) + (s % 3), 2))
    t = PASS_TILES["many_passes"]
    parts.append(_block(t, R, 0, W, np.arange(64), 300) if R == 64 else _block(t, R, 0, W, np.arange(R), 2))
    parts.append(_block(t, R, 17, W, [5, 6], 3))
    t = PASS_TILES["empty_between"]
    for s in (3, 5):
        parts.append(_block(t, R, s, W, np.arange(60), 5))
    for s in (9, 11):
        parts.append(_block(t, R, s, W, [R - 1], 1))
    t = PASS_TILES["marker_first"]
    if R > 700:
        parts.append(_block(t, R, 0, W, [300, 301, 900], 2))
        parts.append(_block(t, R, 3, W, np.arange(63), 4))           # 252 slots, then the run below opens segment 1
        parts.append(_block(t, R, 4, W, [700, R - 1], 1))
    else:
        parts.append(_block(t, R, 0, W, [R - 1], 2))
    t = PASS_TILES["one_group"]
    parts.append(_block(t, R, 6, W, np.arange(64), 4))
    parts.append(_block(t, R, 7, W, [9, 30], 2))
    t = PASS_TILES["long_rows"]
    for r, n in ((3, limit + 1), (R - 1, limit + 700)):
        parts.append((np.full(n, t * R + r), (np.arange(n) * 131) % cols))
    parts.append(_block(t, R, 2, W, np.arange(40), 3))
    rr, cc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rp, ci, va, x = _csr(rows, cols, rr, cc, fold, seed=R + fold)
    lay = layout(rp, ci, cols, W, R, limit, max(4096, W))
    _pass_cache[(R, fold)] = (rows, cols, rp, ci, va, x, lay)
    return _pass_cache[(R, fold)]


def pass_claims(R, lay):
    """Asserts from the model that pass_matrix reaches what its docstring says."""
    P, drow = lay["passes"], lay["drow"]
    t = PASS_TILES["four"]
    assert (lay["cell_len"][:, t] == 4).all()
    assert all(len(P[(t, w)]) == 1 and [n for _, n in P[(t, w)][0]] == [4, 4, 4] for w in range(WAVES))
    t = PASS_TILES["three_segments"]
    assert (lay["cell_len"][:, t] == 100).all()
    assert all([[n for _, n in p] for p in P[(t, w)]] == [[100, 100, 56], [44]] for w in range(WAVES))
    t = PASS_TILES["many_passes"]
    assert len(P[(t, 0)]) > 64 and (t, 5) in P
    t = PASS_TILES["empty_between"]
    assert lay["cell_len"][3, t] >= 256 and lay["cell_len"][4, t] == 0 and lay["cell_len"][5, t] >= 256
    assert lay["cell_len"][9, t] == lay["cell_len"][11, t] and lay["cell_len"][10, t] == 0
    assert sum(n for p in P[(t, 1)] for _, n in p) == lay["cell_len"][3, t] + lay["cell_len"][5, t]
    t = PASS_TILES["marker_first"]
    opened = [(k, int(drow[b])) for p in P[(t, 0)] + P.get((t, 1), []) for k, (b, _) in enumerate(p)]
    assert R <= 700 or ((0, SKIP) in opened and (1, SKIP) in opened), opened
    t = PASS_TILES["one_group"]
    assert [sum(n for _, n in p) for p in P[(t, 2)]] == [256, 4]
    assert lay["long_rows"] == 2
    # every wavefront's passes cover the slots of its runs exactly once, in order
    per_wave = -(-lay["S"] // WAVES)
    for (t, w), mine in P.items():
        want = [np.arange(lay["cell_off"][s, t], lay["cell_off"][s, t] + lay["cell_len"][s, t])
                for s in range(w * per_wave, min(lay["S"], (w + 1) * per_wave))]
        for p in mine:
            assert 1 <= len(p) <= PASS_SEGS and sum(n for _, n in p) <= PASS_SLOTS and all(n % 4 == 0 for _, n in p)
        got = [np.arange(b, b + n) for p in mine for b, n in p]
        assert np.array_equal(np.concatenate(got), np.concatenate(want)), (t, w)


# ------------------------------------------------------------------------------------------ phase 1: the item origin
CHUNK_R, CHUNK_TILES, CHUNK_ITEM = 64, 4, 1024
CHUNK_STRIP_SLOTS = (20, 20, 20, 4, 32, 3000, 1024 + 8)       # per strip
CHUNK_CASES = [(W, fold) for W in (4096, 8192, 16384, 32768) for fold in (False, True)]
_chunk_cache = {}


def chunk_matrix(W, fold):
    """(rows, cols, rp, ci, va, x, layout) at item=1024: strips of 20, 20, 20, 4 and 32 slots, each one cell in one
    tile, put the begins of the phase-1 items at 0, 4, 8 and 12 mod 16 (20, 40, 60), one item shorter than 16 slots
    (at 12 mod 16), one of exactly 32; then a strip of 3000 slots over all tiles, cut into three items at multiples of
    eight, and one of 1032 slots cut into two."""
    if (W, fold) in _chunk_cache:
        return _chunk_cache[(W, fold)]
    R, T = CHUNK_R, CHUNK_TILES
    rows, cols = T * R, len(CHUNK_STRIP_SLOTS) * W
    parts = []
    for s, n in enumerate(CHUNK_STRIP_SLOTS[:5]):
        parts.append(_block(s % T, R, s, W, np.arange(n // 4) * 2 + s, 4))
    parts.append(_block(0, R, 5, W, np.arange(60), 13))                # 780
    parts.append(_block(1, R, 5, W, np.arange(64), 12))                # 768
    parts.append(_block(2, R, 5, W, np.arange(64), 11))                # 704
    parts.append(_block(3, R, 5, W, np.arange(44), 17))                # 748
    parts.append(_block(1, R, 6, W, np.arange(64), 16))                # 1024
    parts.append(_block(2, R, 6, W, [0, 63], 4))                       # 8
    rr, cc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rp, ci, va, x = _csr(rows, cols, rr, cc, fold, seed=W + fold)
    lay = layout(rp, ci, cols, W, R, ed.default_long_row(len(CHUNK_STRIP_SLOTS)), CHUNK_ITEM)
    _chunk_cache[(W, fold)] = (rows, cols, rp, ci, va, x, lay)
    return _chunk_cache[(W, fold)]


def chunk_claims(lay):
    strip_slots = lay["cell_len"].sum(axis=1)
    assert tuple(int(v) for v in strip_slots) == CHUNK_STRIP_SLOTS
    items = lay["items"]
    begins = {b % 16 for _, b, _ in items}
    assert begins == {0, 4, 8, 12}, begins
    assert any(e - b < 16 and b % 16 == 12 for _, b, e in items)                  # shorter than one chunk, unaligned
    assert any(e - b == 32 and b % 16 == 0 for _, b, e in items)                  # exactly 16 k slots
    assert any((e - b) % 16 == 0 and b % 16 == 8 for _, b, e in items)            # 16 k slots from an unaligned begin
    assert sum(s == 5 for s, _, _ in items) == 3 and sum(s == 6 for s, _, _ in items) == 2
    assert any(b % 16 == 8 and s == 5 and b != int(lay["cell_off"][5, 0]) for s, b, _ in items)   # a cut inside a strip
    single = [(lay["cell_len"][s] > 0).sum() for s in range(5)]
    assert single == [1] * 5                                                      # strips holding a single cell
    assert lay["long_rows"] == 0
