"""What tests/build_edge_cases.py generates has the length, the tile position or the defect position it is named for, and
the host twins agree with its numpy references on the same cases (no GPU): tests/test_gpu_build_edges.py runs these
cases against the device builders."""
import numpy as np
import pytest

import build_edge_cases as bc
import fsai_cases as fc
import mis2_cases as mc
import reorder_cases as rc
from spgemm_cases import assert_same

TILE = bc.TILE


def _same(got, want, what):
    for g, w, part in zip(got, want, ("row_ptrs", "col_indices", "values")):
        assert np.asarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, part)


# ---- the scan's geometry ------------------------------------------------------------------------------------------
def test_scan_levels_recomputed_from_the_tile_size():
    assert bc.scan_levels(TILE * TILE) == [16_777_216, 4096, 1]
    assert bc.scan_levels(TILE * TILE + 1) == [16_777_217, 4097, 2, 1]
    assert [bc.scan_launches(bc.scan_levels(n)) for n in (1, 2, TILE, TILE + 1, TILE * TILE, TILE * TILE + 1)] == \
        [1, 1, 1, 3, 3, 5]
    assert [bc.scan_depth(n) for n in (1, TILE, TILE + 1, TILE * TILE, TILE * TILE + 1)] == [1, 1, 2, 2, 3]
    for n in (1, 2, TILE, TILE + 1, 3 * TILE + 1, TILE * TILE, TILE * TILE + 1):
        levels = bc.scan_levels(n)
        assert levels[0] == n and levels[-1] == 1
        assert all(levels[l + 1] == -(-levels[l] // TILE) for l in range(len(levels) - 1))
        # every level below the top writes one total per tile, each behind the last level's
        assert bc.scan_sums(levels) >= sum(-(-size // TILE) for size in levels[:max(1, len(levels) - 1)])


def test_the_scanned_lengths_are_the_ones_named():
    assert [r + 1 for r in bc.SCAN_ROWS] == [4095, 4096, 4097, 8192, 8193, 3 * 4096 + 1]
    assert [bc.scan_depth(r + 1) for r in bc.SCAN_ROWS] == [1, 1, 2, 2, 2, 2]
    assert [r + 1 for r in bc.THIRD_LEVEL_ROWS] == [TILE * TILE, TILE * TILE + 1]
    assert [bc.scan_depth(r + 1) for r in bc.THIRD_LEVEL_ROWS] == [2, 3]
    assert [bc.SEGMENTS * m + 1 for m in bc.SPGEMM_ROWS[:4]] == [4093, 4099, 8191, 8197]
    assert [m + 1 for m in bc.SPGEMM_ROWS[4:]] == [4096, 4097]
    assert [bc.SEGMENTS * m + 1 for m in bc.SPGEMM_THIRD_LEVEL_ROWS] == [16_777_213, 16_777_219]
    assert [bc.scan_depth(bc.SEGMENTS * m + 1) for m in bc.SPGEMM_THIRD_LEVEL_ROWS] == [2, 3]
    assert [bc.scan_depth(n + 1) for n in bc.FSAI_ROWS] == [1, 2, 2] == [bc.scan_depth(n + 1) for n in bc.MIS2_ROWS]
    assert [bc.scan_depth(t + 1) for t in bc.COO_TRIPLETS] == [1, 2, 2, 2]
    tiles = [-(-nnz // TILE) for nnz in bc.TRANSPOSE_NNZ]
    assert tiles == [16, 17, 18] and [256 * t for t in tiles] == [4096, 4352, 4608]
    assert [bc.scan_depth(256 * t) for t in tiles] == [1, 2, 2]


# ---- edge_profile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", bc.SCAN_ROWS + bc.THIRD_LEVEL_ROWS + (600_000,))
def test_edge_profile_has_its_four_properties(rows):
    for seed in (1, 2):
        lengths = bc.edge_profile(rows, seed=seed)
        assert lengths.size == rows and lengths.min() == 0 and lengths.max() <= 3 and lengths.dtype == np.int32
        hole = bc.empty_tile(rows)
        inside = (lambda at: at // TILE == hole) if hole is not None else (lambda at: np.zeros(at.shape, bool))
        # (a) the borders
        borders = bc.border_rows(rows)
        k = np.arange(TILE, rows + 1, TILE)
        named = np.concatenate([[0, rows - 1], k - 2, k - 1, k, k + 1])
        assert k.size == rows // TILE and np.isin(named[named < rows], borders).all()
        assert np.all(lengths[borders[~inside(borders)]] > 0)
        # (b) an empty tile with a non-empty one behind it
        totals = bc.tile_totals(lengths)
        assert totals.size == -(-(rows + 1) // TILE)
        if rows >= 3 * TILE:
            assert hole == 1 and totals[hole] == 0 and totals[hole - 1] > 0 and totals[hole + 1] > 0
            assert not lengths[hole * TILE:(hole + 1) * TILE].any()
        else:
            assert hole is None
        # (c) neighbouring totals differ
        assert np.all(np.diff(totals) != 0)
        # (d) the stride, and with it every in-tile offset
        sprinkled = bc.sprinkle_rows(rows)
        assert np.gcd(bc.SPRINKLE, TILE) == 1 and np.all(lengths[sprinkled[~inside(sprinkled)]] > 0)
        if rows >= TILE * TILE:
            assert np.unique(np.flatnonzero(lengths) % TILE).size == TILE
        # few entries: the rows are what matter
        assert lengths.sum() <= 3 * (borders.size + sprinkled.size + 2 * totals.size)
        rp = bc.row_ptrs_of(lengths)
        assert rp.dtype == np.int32 and rp[0] == 0 and rp[-1] == lengths.sum()


def test_the_total_stands_alone_in_the_second_tile_at_4096_rows():
    totals = bc.tile_totals(bc.edge_profile(4096))
    assert totals.size == 2 and totals[1] == 0 and totals[0] > 0
    assert bc.tile_totals(bc.edge_profile(4095)).size == 1
    totals = bc.tile_totals(bc.edge_profile(TILE * TILE))
    assert totals.size == TILE + 1 and totals[-1] == 0 and totals[-2] > 0          # and alone in level 1's second tile


# ---- the references against the loop definitions and the host twins ---------------------------------------------------
@pytest.mark.parametrize("rows", bc.SCAN_ROWS)
def test_sum_structure_equals_the_host_twin(spmv, rows):
    import csr_ops_cases as oc
    a, b = bc.add_pair(rows)
    assert a[0].size == rows + 1 and np.all(np.diff(a[0]) <= 3)
    common = np.intersect1d(bc.rows_of(a[0]).astype(np.int64) * 16 + a[1], bc.rows_of(b[0]).astype(np.int64) * 16 + b[1]).size
    status, want = oc.host_sum(spmv, rows, 16, 1.5, a, -0.75, b)
    assert status == 0
    rp, ci = bc.np_add_structure(rows, 16, a, b)
    assert rp.tobytes() == want[0].tobytes() and ci.tobytes() == want[1].tobytes()
    assert rows < 8191 or 0 < common < min(a[1].size, b[1].size)                   # some columns shared, not all
    if rows == 4094:
        assert_same(want, oc.add_loop(rows, 1.5, a, -0.75, b), "the loop definition")


@pytest.mark.parametrize("rows", bc.SCAN_ROWS)
def test_row_permutation_equals_the_host_twin(spmv, rows):
    a = bc.short_rows_from(bc.edge_profile(rows, seed=4), 14)
    reversal = np.arange(rows, dtype=np.int32)[::-1].copy()
    A, B = spmv.csr_from_arrays(rows, 16, *a), spmv.csr_create(0, 0, 0)
    for perm in (reversal, None):
        assert spmv.csr_permute_cpu(B, A, perm, None) == 0
        want = bc.np_permute_rows(a, np.arange(rows) if perm is None else perm)
        _same(spmv.csr_host_arrays(B), want, ("permute", rows))
    # the reversal moves the rows with entries across the tile borders: row k tile - 2 becomes row rows + 1 - k tile
    got = np.diff(bc.np_permute_rows(a, reversal)[0])
    assert np.array_equal(got, np.diff(a[0])[::-1])
    if rows >= 8191:
        assert not np.array_equal(got, np.diff(a[0])) and got[rows + 1 - TILE] > 0 and (rows + 1 - TILE) // TILE != 0
    if rows == 4094:
        _same(bc.np_permute_rows(a, reversal), rc.permute(rows, 16, *a, reversal, None), "the loop definition")
    spmv.csr_destroy(A)
    spmv.csr_destroy(B)


@pytest.mark.parametrize("m", bc.SPGEMM_ROWS)
def test_product_structure_equals_the_host_twin(spmv, m):
    import spgemm_cases as sc
    a, b = bc.product_pair(m)
    bound = bc.product_bounds(a, b)
    assert (bound == 0).any() and ((bound > 0) & (bound <= 16)).any() and (bound > 16).any()   # three classes
    status, want = sc.host_product(spmv, m, 16, 64, a, b)
    assert status == 0
    rp, ci = bc.np_product_structure(m, 64, a, b)
    assert rp.tobytes() == want[0].tobytes() and ci.tobytes() == want[1].tobytes()
    if m == 682:
        assert_same(want, sc.product_loop(m, 64, a, b), "the loop definition")


@pytest.mark.parametrize("count", bc.COO_TRIPLETS)
def test_triplets_hold_duplicates_and_their_structure_equals_the_host_twin(spmv, count):
    import assemble_cases as ac
    r, c, v = bc.coo_triplets(count)
    assert r.size == c.size == v.size == count
    C = spmv.csr_create(0, 0, 0)
    assert spmv.csr_from_coo_cpu(C, 700, 40, r, c, v) == 0
    want = spmv.csr_host_arrays(C)
    spmv.csr_destroy(C)
    rp, ci = bc.np_coo_sum_structure(700, 40, r, c)
    assert rp.tobytes() == want[0].tobytes() and ci.tobytes() == want[1].tobytes()
    assert count // 4 <= count - ci.size <= count // 3
    if count == 4095:
        assert ac.same(want, ac.assemble(700, 40, r, c, v))


def test_fsai_and_mis2_inputs_have_the_rows_named(spmv):
    for n in bc.FSAI_ROWS[:1]:
        m, rp, ci, va = fc.banded_spd(n, 2)
        assert m == n and rp.size == n + 1 and np.diff(rp).max() == 5
    n, rp, ci, va = mc.path_equal(8192)
    assert n == 8192 and rp[-1] == 3 * n - 2
    A = spmv.csr_from_arrays(n, n, rp, ci, va)
    status, agg, count, _ = spmv.amg_aggregate_mis2_cpu_csr(A, 0.08, 0)
    spmv.csr_destroy(A)
    assert status == 0
    roots = np.flatnonzero(np.diff(np.concatenate([[-1], np.sort(agg)])))         # (count aggregates, all used)
    assert roots.size == count and agg.min() == 0 and agg.max() == count - 1
    # aggregates on both sides of both tile borders of the scan over the root flags
    for border in (4096, 8192):
        assert (agg[:border] < agg[border - 1]).any() and agg[border - 1] >= 1
    assert agg[4095] < agg[8191] and np.all(np.diff(agg.astype(np.int64)) >= 0)


@pytest.mark.parametrize("nnz", bc.TRANSPOSE_NNZ)
def test_transpose_cases_have_the_entries_and_digits_named(nnz):
    for passes in (0, 1, 2, 3):
        rows, cols, (rp, ci, va) = bc.transpose_case(nnz, passes)
        assert rp.size == rows + 1 and rp[-1] == nnz == ci.size and ci.min() >= 0 and ci.max() < cols
        differ = np.bitwise_or.reduce(ci ^ ci[0])
        assert sum(1 for d in range(4) if (differ >> (8 * d)) & 255) == passes == bc.radix_passes(cols)
        t_rp, t_ci, t_va = bc.np_transpose(rows, cols, rp, ci, va)
        assert t_rp[-1] == nnz and np.all(np.diff(t_ci.astype(np.int64))[np.diff(np.sort(ci, kind="stable")) == 0] >= 0)


# ---- row_of -------------------------------------------------------------------------------------------------------
def test_row_of_shapes_sit_on_the_workgroup_edges():
    shapes = bc.ROW_OF_SHAPES
    for nnz in (1, 255, 256, 257, 511, 512, 513):
        assert shapes[f"{nnz} in one row"].tolist() == [nnz] and shapes[f"{nnz} rows of one"].tolist() == [1] * nnz
    for end in (255, 256, 257):
        assert end in bc.row_ends(shapes[f"a row ends on entry {end}"]).tolist()
    long = shapes["a row of 1000 between rows of one"]
    rp = bc.row_ptrs_of(long)
    whole = [g for g in range(-(-int(rp[-1]) // bc.GROUP)) if rp[1] <= g * bc.GROUP and (g + 1) * bc.GROUP <= rp[2]]
    assert len(whole) >= 2 and -(-int(rp[-1]) // bc.GROUP) == 4       # workgroups that lie inside the one row
    gap = shapes["600 empty rows inside one workgroup"]
    rp = bc.row_ptrs_of(gap)
    assert rp[2] == 101 and np.all(gap[2:602] == 0) and rp[602] == 101 and rp[-1] <= bc.GROUP
    ends = shapes["300 empty rows at either end"]
    assert not ends[:300].any() and not ends[-300:].any() and ends[300] > 0 and ends[-301] > 0
    assert shapes["one row"].size == 1
    starts = bc.row_ptrs_of(shapes["rows that start at multiples of 256"])[:-1][shapes["rows that start at multiples of 256"] > 0]
    assert np.all(starts % bc.GROUP == 0) and starts.size == 4
    for name, lengths in shapes.items():
        rp = bc.row_ptrs_of(lengths)
        want = np.repeat(np.arange(lengths.size), lengths)
        assert np.array_equal(bc.rows_of(rp), want), name
        assert np.all(rp[want] <= np.arange(want.size)) and np.all(np.arange(want.size) < rp[want + 1]), name


# ---- the structure check ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["entries", "rows"])
def test_validate_defects_sit_where_only_the_named_work_item_sees_them(regime):
    rp, ci, va = bc.validate_matrix(regime)
    rows, nnz = bc.VALIDATE_ROWS, ci.size
    assert rp.size == rows + 1 and bc.is_valid(rp, ci, bc.VALIDATE_COLS, nnz)
    assert (680_000 < nnz < 720_000 and nnz > rows + 1) if regime == "entries" else (900 < nnz < 1100)
    assert bc.VALIDATE_ITEMS == 524_288 < rows - 1
    defects = bc.validate_defects(rp, ci)
    assert len(defects) == (12 if regime == "entries" else 10)
    seen = {}
    for name, defect in defects.items():
        bad_rp, bad_ci = bc.with_defect(rp, ci, defect)
        assert not bc.is_valid(bad_rp, bad_ci, bc.VALIDATE_COLS, nnz), name
        items = bc.items_that_see(bad_rp, bad_ci, bc.VALIDATE_COLS, nnz)
        assert len(items) == 1, (name, items)                     # nothing else gives the defect away
        seen[name] = items[0]
    assert seen["row_ptrs[0] = 1"] == 0 and seen["row_ptrs[rows] = nnz - 1"] == rows == seen["row_ptrs[rows] = nnz + 1"]
    assert [seen[f"a decrease at row {r}"] for r in (1, 524_288, rows - 1)] == [1, 524_288, rows - 1]
    assert seen["column -1 at entry 0"] == 0 == seen["column = cols at entry 0"]
    assert seen[f"column -1 at entry {nnz - 1}"] == nnz - 1
    if regime == "entries":
        assert seen["column -1 at entry 524288"] == 524_288 == seen["column = cols at entry 524288"]
        assert all(seen[name] >= bc.VALIDATE_ITEMS for name in bc.DOOR_DEFECTS)    # past the first trip
        assert max(seen.values()) == nnz - 1 > rows                               # the entries' own tail
    else:
        assert max(seen.values()) == rows > nnz                                   # the row pointers' own tail


# ---- iota ---------------------------------------------------------------------------------------------------------
def test_ordering_size_makes_a_second_trip_of_iota():
    n = bc.IOTA_ITEMS + 257
    assert bc.IOTA_ITEMS == 262_144 and n + 1 > bc.IOTA_ITEMS
    perm, inverse, color_ptr = rc.ordering(np.arange(n) % 3, 3)
    assert color_ptr.tolist() == [0, -(-n // 3), -(-n // 3) + -(-(n - 1) // 3), n]
    assert np.array_equal(perm[:3], [0, 3, 6]) and np.array_equal(inverse[perm], np.arange(n))
