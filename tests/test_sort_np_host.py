"""tests/sort_np.py on hand-made inputs, without a GPU: the restated geometry (band units, odd tile counts, a last
tile row that is cut off), the clamp of border-ring cells, the counts per (unit, K1 workgroup), the item numbering of
both sorts, and the rounding of the option bin_batch as pass_plan.cpp has it."""
import os
import re

import numpy as np

import sort_np as snp

CSRC = os.path.join(os.path.dirname(__file__), "..", "slicer_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def coords(g, npix):
    """f32 coordinates in the middle of cell g (g = -1 and npix: the border ring)."""
    return ((np.asarray(g, np.float64) + 0.5) / npix).astype(np.float32)


def test_constants_are_the_kernels():
    sort, kern, plan = source("slicer_sort.hip"), source("slicer_kernels.hpp"), source("pass_plan.cpp")
    for text, names in ((sort, dict(kScanBins=snp.SCAN_BINS, kKeep=snp.SCAN_KEEP, kSortBatch=snp.SORT_BATCH,
                                    kS2Cap=snp.S2_CAP, kS2MaxMine=snp.S2_MAX_MINE)),
                        (kern, dict(kMaxUnits=snp.MAX_UNITS, kMaxBins=snp.MAX_BINS, kSubBatches=snp.SUB_BATCHES,
                                    kSort2Blocks=snp.SORT2_BLOCKS, kMaxCoarse=snp.MAX_COARSE,
                                    kMaxCoarseTiles=snp.MAX_COARSE_TILES, kMaxSortGroups=snp.MAX_SORT_GROUPS)),
                        (plan, dict(kUnitBins=snp.UNIT_BINS))):
        for name, value in names.items():
            assert re.search(rf"constexpr int {name} = {value};", text), name
    assert "#define SLICER_K3_BLOCK 512" in sort and "#define SLICER_K3_STAGE 4096" in sort
    assert "constexpr int kScanSegs = 1024 / kScanBins;" in sort and snp.SCAN_SEGS == 1024 // snp.SCAN_BINS


def test_bin_batch_rounding_is_pass_plan_s():
    plan = source("pass_plan.cpp")
    # the two statements option_batch restates; if they change, so must it
    assert "G.batch = env_b ? std::min(std::max((env_b / 1024) * 1024, 1024), 64512) : kBinBatch;" in plan
    assert "G.batch = std::min(G.batch, std::max(1024, 65535 / reps / 1024 * 1024));" in plan
    assert "int rep_windows(int nrmax) { return (2 * nrmax + 1 + 6) / 7; }" in plan
    for asked, reps, want in ((1024, 1, 1024), (1, 1, 1024), (1023, 1, 1024), (2047, 1, 1024), (2048, 1, 2048),
                              (32768, 1, 32768), (64512, 1, 64512), (65535, 1, 64512), (1 << 20, 1, 64512),
                              (32768, 9, 7168), (4096, 9, 4096), (32768, 25, 2048), (32768, 49, 1024), (1024, 49, 1024)):
        assert snp.option_batch(asked, reps) == want, (asked, reps)
    assert [snp.rep_window_side(n) for n in (0, 1, 2, 3, 4, 6, 7)] == [1, 3, 5, 7, 5, 7, 5]
    G = snp.geom(64, 1, 4, 4, 32768, nrep=1)
    assert (G.reps, G.batch, G.region) == (9, 7168, 9 * 7168)


def test_whole_plane_units_and_an_odd_tile_count():
    G = snp.geom(48, 3, 4, 4, 32768)
    assert (G.ntx, G.nty, G.units_per_plane, G.rows_per_unit, G.tiles_per_unit, G.n_units, G.nbins) == (3, 3, 1, 3, 9, 3, 27)
    unit, tile = snp.cell_to_tile([0, 47, 16, 47], [0, 47, 31, 0], [0, 0, 1, 2], G)
    assert list(unit) == [0, 0, 1, 2] and list(tile) == [0, 8, 4, 2]


def test_band_units_and_a_cut_last_band():
    G = snp.geom(520, 4, 3, 3, 32768)  # 65 x 65 tiles of 8 x 8: 16900 bins > kUnitBins -> bands of 2048 // 65 = 31 rows
    assert (G.ntx, G.nty, G.rows_per_unit, G.units_per_plane, G.tiles_per_unit, G.n_units, G.nbins) == \
        (65, 65, 31, 3, 2015, 12, 24180)
    # pixel rows 0, 247 (tile row 30), 248 (31), 512 (64: the third row of the last band, which has 3 of 31)
    unit, tile = snp.cell_to_tile([0, 519, 8, 519], [0, 247, 248, 512], [0, 0, 1, 3], G)
    assert list(unit) == [0, 0, 4, 11] and list(tile) == [0, 30 * 65 + 64, 1, 2 * 65 + 64]
    assert 2 * 65 + 64 < G.tiles_per_unit - 1  # the last band's bins past its three rows stay empty
    # forced thin bands; a request below what kMaxUnits allows is raised
    G = snp.geom(520, 4, 3, 3, 1024, unit_rows=13)
    assert (G.rows_per_unit, G.units_per_plane, G.tiles_per_unit, G.n_units, G.nbins) == (13, 5, 845, 20, 16900)
    G = snp.geom(96, 4, 4, 4, 1024, unit_rows=4)
    assert (G.nty, G.rows_per_unit, G.units_per_plane, G.tiles_per_unit, G.n_units) == (6, 4, 2, 24, 8)
    unit, tile = snp.cell_to_tile([95], [95], [3], G)
    assert list(unit) == [7] and list(tile) == [1 * 6 + 5]
    G = snp.geom(128, 4, 3, 3, 1024, unit_rows=1)
    assert (G.rows_per_unit, G.units_per_plane, G.n_units) == (2, 8, 32)
    G = snp.geom(96, 4, 4, 4, 1024, unit_rows=100)  # more rows than the map has: one band
    assert (G.rows_per_unit, G.units_per_plane) == (6, 1)


def test_a_last_tile_row_and_column_that_are_cut_off():
    G = snp.geom(100, 1, 5, 4, 1024)  # 32 x 16 tiles: 4 columns (the last 4 pixels wide), 7 rows (the last 4 high)
    assert (G.ntx, G.nty, G.tiles_per_unit) == (4, 7, 28)
    unit, tile = snp.cell_to_tile([95, 96, 99, 0], [95, 96, 99, 96], 0, G)
    assert list(unit) == [0] * 4 and list(tile) == [5 * 4 + 2, 6 * 4 + 3, 27, 24]


def test_border_ring_cells_are_clamped_and_ngp_drops_them():
    npix = 64
    G = snp.geom(npix, 1, 4, 4, 1024)
    gx = np.array([-1, 0, 63, 64, -1, 64, 10])
    gy = np.array([5, -1, 64, 63, -1, 64, 10])
    cx, cy = snp.centre_cells(coords(gx, npix), coords(gy, npix), npix)
    assert np.array_equal(cx, gx) and np.array_equal(cy, gy)
    unit, tile = snp.cell_to_tile(gx, gy, 0, G)
    assert list(tile) == [0, 0, 15, 15, 0, 15, 0] and not unit.any()
    entries = [(coords(gx, npix), coords(gy, npix), np.arange(7))]
    tsc, ngp = snp.Chunk(G, entries, 7, ngp=False), snp.Chunk(G, entries, 7, ngp=True)
    assert tsc.count.tolist() == [[7]] and ngp.count.tolist() == [[1]]
    assert tsc.tile_counts(0, 0)[[0, 15]].tolist() == [4, 3] and ngp.tile_counts(0, 0)[0] == 1


def test_counts_per_unit_and_workgroup():
    npix = 48
    G = snp.geom(npix, 3, 4, 4, 1024)
    rng = np.random.default_rng(1)
    n = 2 * 1024 + 100
    plane = rng.integers(0, 3, n)
    gx, gy = rng.integers(0, npix, n), rng.integers(0, npix, n)
    entries = [(coords(gx[plane == p], npix), coords(gy[plane == p], npix), np.nonzero(plane == p)[0]) for p in range(3)]
    c = snp.Chunk(G, entries, n, ngp=False)
    assert c.nblocks == 3 and c.count.shape == (3, 3) and c.count.sum() == n
    for p in range(3):
        for w in range(3):
            sel = (plane == p) & (np.arange(n) // 1024 == w)
            assert c.count[p, w] == sel.sum()
            want = np.bincount((gy[sel] // 16) * 3 + gx[sel] // 16, minlength=9)
            assert np.array_equal(c.tile_counts(p, w), want)
            assert np.array_equal(c.hist()[w, 9 * p:9 * p + 9], want)
            assert c.k3_single(p, w) == (p != 1)  # unit 1 starts at bin 9: not word-aligned in the u16 histogram
    assert np.array_equal(c.records, np.bincount(plane, minlength=3))
    assert c.scan_groups() == 1 and c.scan_rows_per_lane() == 1 and c.scan_idle_segments() == 29


def test_k3_item_numbering_covers_every_pair_once():
    G = snp.geom(64, 4, 4, 4, 1024)
    for nblocks in (1, 7, 8, 19, 67):
        c = snp.Chunk(G, [(np.zeros(0, np.float32),) * 2 + (np.zeros(0, np.int64),)] * 4, nblocks * 1024, ngp=False)
        assert c.nblocks == nblocks and c.k3_items() == 4 * 8 * ((nblocks + 7) // 8)
        pairs = [c.k3_item(i) for i in range(c.k3_items())]
        assert len(set(pairs)) == len(pairs)
        assert {p for p in pairs if p[1] < nblocks} == {(u, w) for u in range(4) for w in range(nblocks)}
        assert sum(1 for p in pairs if p[1] >= nblocks) == 4 * (-nblocks % 8)
    assert c.k3_workgroups(256, 1) == 256 and c.k3_workgroups(256, 2) == 288 and c.k3_workgroups(4, 1) == 8
    assert c.k3_workgroups(100, 1) == 96


def test_sub_batches_and_staging_rounds():
    assert snp.sub_batches(30000) == [8192, 8192, 8192, 5424] and snp.staging_rounds(5424) == 2
    assert snp.sub_batches(8192) == [8192] and snp.sub_batches(8193) == [8192, 1] and snp.sub_batches(0) == []
    assert [snp.staging_rounds(n) for n in (1, 4096, 4097, 8192)] == [1, 1, 2, 2]


def test_two_level_sort_units():
    G2 = snp.sort2_geom(snp.geom(128, 4, 3, 3, 4096))  # 16 tile rows x 4 planes: 64 units of one row
    assert (G2.crow_log2, G2.n_units, G2.tiles_per_unit) == (0, 64, 16)
    G2 = snp.sort2_geom(snp.geom(520, 4, 3, 3, 4096))  # 260 rows: pairs of rows, then 4 x 65 tiles would pass 256
    assert (G2.crow_log2, G2.units_per_plane, G2.n_units, G2.tiles_per_unit) == (1, 33, 132, 130)
    G2 = snp.sort2_geom(snp.geom(512, 4, 3, 3, 4096))
    assert (G2.crow_log2, G2.n_units, G2.tiles_per_unit) == (2, 64, 256)
    G2 = snp.sort2_geom(snp.geom(256, 1, 5, 5, 32768))
    assert (G2.crow_log2, G2.n_units, G2.tiles_per_unit) == (0, 8, 8)
    assert snp.sort2_geom(snp.geom(256, 1, 5, 5, 33792)) is None  # batch above 32768
    assert snp.sort2_geom(snp.geom(64, 1, 4, 4, 1024, nrep=1)) is None  # replication
    # item totals: unit = band of 2^crow_log2 tile rows, group = 16 K1 workgroups
    G2 = snp.sort2_geom(snp.geom(520, 4, 3, 3, 1024))
    n = 17 * 1024
    gy = np.full(n, 519)
    gy[:1024] = 16  # workgroup 0: tile row 2 -> band 1; the others: tile row 64 -> band 32
    entries = [(coords(np.zeros(n), 520), coords(gy, 520), np.arange(n))] + [(np.zeros(0, np.float32),) * 2 + (np.zeros(0, np.int64),)] * 3
    c = snp.Chunk(G2, entries, n, ngp=False)
    tot = c.sort2_item_totals()
    assert c.sort2_groups() == 2 and tot.shape == (2, 132) and tot.sum() == n
    assert tot[0, 1] == 1024 and tot[0, 32] == 15 * 1024 and tot[1, 32] == 1024
    assert c.sort2_workgroups(256, 1) == 256 and c.sort2_workgroups(2, 1) == 8 and c.sort2_qualifies()
    assert snp.Chunk(G2, entries, 513 * 1024, ngp=False).sort2_groups() == 33
