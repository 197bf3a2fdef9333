"""Restatement of the bookkeeping between project+bin (K1) and the sorts of the binned path -- k_scan_blocks (K2),
k_bin_scatter (K3) and k_sort2 (K3') of slicer_amd/csrc/slicer_sort.hip -- in numpy.  TEST INFRASTRUCTURE ONLY:
tests/test_gpu_sort.py states with it, before the GPU is called, which branch of those kernels a case reaches;
tests/test_sort_np_host.py keeps it honest without a GPU.

The geometry is the one choose_geom (pass_plan.cpp) derives when the handle's options force it: tile_log2, tile_h_log2
and bin_batch are always given here, unit_rows where bands are asked for.  Records are the oracle's selected entries
with their particle index (oracle.select_project(..., want_index=True)): the K1 workgroup of a record is its index
inside the deposit call // batch, its unit and tile-in-unit are cell_to_tile (slicer_binned_common.hpp) of the clamped
centre pixel.  Nothing here looks at the order in which K1 stores the records of one workgroup.
"""
from types import SimpleNamespace

import numpy as np

# slicer_kernels.hpp, pass_plan.cpp
UNIT_BINS, MAX_UNITS, MAX_BINS = 8192, 32, 32768
# slicer_sort.hip: K2
SCAN_BINS, SCAN_SEGS, SCAN_KEEP = 32, 32, 16
# slicer_sort.hip: K3
SORT_BLOCK, SORT_BATCH, SORT_STAGE = 512, 8192, 4096
# slicer_sort.hip / slicer_kernels.hpp: K3'
S2_CAP, S2_MAX_MINE = 8192, 64
SUB_BATCHES, SORT2_BLOCKS, MAX_COARSE, MAX_COARSE_TILES, MAX_SORT_GROUPS = 16, 16, 256, 256, 32
SORT2_SLOTS = SORT2_BLOCKS * SUB_BATCHES


def cdiv(a, b):
    return (a + b - 1) // b


# ---- geometry ---------------------------------------------------------------------------------------------------
def rep_window_side(nrmax):
    windows = (2 * nrmax + 1 + 6) // 7
    return cdiv(2 * nrmax + 1, windows)


def option_batch(bin_batch, reps=1):
    """Particles per K1 workgroup for a forced option bin_batch > 0 (choose_geom)."""
    assert bin_batch > 0, "the tests force bin_batch: 0 lets the chunk size choose"
    batch = min(max(bin_batch // 1024 * 1024, 1024), 64512)
    return min(batch, max(1024, 65535 // reps // 1024 * 1024))


def geom(npix, n_planes, tile_log2, tile_h_log2, bin_batch, unit_rows=0, nrep=0):
    """choose_geom with tile_log2, tile_h_log2 and bin_batch forced."""
    assert tile_log2 and tile_h_log2 and 3 <= tile_log2 <= 8 and 3 <= tile_h_log2 <= 8
    G = SimpleNamespace(npix=npix, n_planes=n_planes, tw_log2=tile_log2, th_log2=tile_h_log2)
    G.ntx = (npix + (1 << G.tw_log2) - 1) >> G.tw_log2
    G.nty = (npix + (1 << G.th_log2) - 1) >> G.th_log2
    if G.ntx * G.nty * n_planes <= UNIT_BINS and not unit_rows:
        G.units_per_plane, G.rows_per_unit = 1, G.nty
    else:
        rows = min(unit_rows, G.nty) if unit_rows else max(1, 2048 // G.ntx)
        max_upp = max(1, MAX_UNITS // n_planes)
        G.rows_per_unit = max(rows, cdiv(G.nty, max_upp))
        G.units_per_plane = cdiv(G.nty, G.rows_per_unit)
    G.tiles_per_unit = G.rows_per_unit * G.ntx
    G.n_units = n_planes * G.units_per_plane
    G.nbins = G.n_units * G.tiles_per_unit
    assert G.n_units <= MAX_UNITS and G.tiles_per_unit <= 8192 and G.nbins <= MAX_BINS, "the binned path refuses this pass"
    side = rep_window_side(nrep)
    G.reps = side * side
    G.batch = option_batch(bin_batch, G.reps)
    G.region = G.batch * G.reps
    return G


def sort2_geom(G):
    """The units of the two-level sort (sort2_geom, binned_pass.cpp): bands of 2^crow_log2 tile rows; None where the
    pass does not fit."""
    def units(cl):
        return G.n_planes * ((G.nty + (1 << cl) - 1) >> cl)
    cl = 0
    while units(cl) > 64 and (2 << cl) * G.ntx <= MAX_COARSE_TILES:
        cl += 1
    G2 = SimpleNamespace(**vars(G))
    G2.crow_log2 = cl
    G2.rows_per_unit = 1 << cl
    G2.units_per_plane = cdiv(G.nty, G2.rows_per_unit)
    G2.tiles_per_unit = G2.rows_per_unit * G.ntx
    G2.n_units = G.n_planes * G2.units_per_plane
    G2.nbins = G2.n_units * G2.tiles_per_unit
    ok = G2.n_units <= MAX_COARSE and G2.tiles_per_unit <= MAX_COARSE_TILES and G.region == G.batch and G.batch <= 32768
    return G2 if ok else None


def centre_cells(xs, ys, npix):
    """utilities.cpp:69-70: the cell of a coordinate is floor(x / dl) in doubles, dl = 1 / npix."""
    dl = 1.0 / np.float64(npix)
    return (np.floor(np.asarray(xs, np.float32).astype(np.float64) / dl).astype(np.int64),
            np.floor(np.asarray(ys, np.float32).astype(np.float64) / dl).astype(np.int64))


def cell_to_tile(gx, gy, plane, G):
    """(unit, tile-in-unit) of the centre cell, clamped into the map first (border-ring entries of TSC feed the edge
    pixels and are binned with the clamped cell)."""
    gx = np.clip(np.asarray(gx, np.int64), 0, G.npix - 1)
    gy = np.clip(np.asarray(gy, np.int64), 0, G.npix - 1)
    ty, tx = gy >> G.th_log2, gx >> G.tw_log2
    band = ty // G.rows_per_unit if G.units_per_plane > 1 else np.zeros_like(ty)
    trow = ty - band * G.rows_per_unit
    return np.asarray(plane, np.int64) * G.units_per_plane + band, trow * G.ntx + tx


# ---- one deposit call through K1 .. K3 --------------------------------------------------------------------------
class Chunk:
    """The records one deposit call of n particles hands from K1 to the sorts.

    entries: per plane (xs, ys, index), index counted from the call's first particle (the oracle's selected entries;
    lateral replicas share their particle's index).  NGP emits no record for an entry centred off the map."""

    def __init__(self, G, entries, n, ngp):
        self.G, self.n = G, n
        self.nblocks = cdiv(n, G.batch)
        plane, gx, gy, idx = [], [], [], []
        for p, (xs, ys, index) in enumerate(entries):
            cx, cy = centre_cells(xs, ys, G.npix)
            keep = np.ones(len(cx), bool)
            if ngp:
                keep = (cx >= 0) & (cx < G.npix) & (cy >= 0) & (cy < G.npix)
            plane.append(np.full(int(keep.sum()), p, np.int64))
            gx.append(cx[keep])
            gy.append(cy[keep])
            idx.append(np.asarray(index, np.int64)[keep])
        self.plane, self.gx, self.gy, self.index = (np.concatenate(a) for a in (plane, gx, gy, idx))
        assert self.index.min(initial=0) >= 0 and self.index.max(initial=0) < n
        self.wg = self.index // G.batch
        self.unit, self.tile = cell_to_tile(self.gx, self.gy, self.plane, G)
        self.bin = self.unit * G.tiles_per_unit + self.tile
        # bcount[unit][workgroup]; hist[workgroup][bin] (K1's u16 rows: a count fits because region <= 65535)
        self.count = np.bincount(self.unit * self.nblocks + self.wg,
                                 minlength=G.n_units * self.nblocks).reshape(G.n_units, self.nblocks)
        assert self.count.max(initial=0) <= G.region <= 65535
        self.records = np.bincount(self.plane, minlength=G.n_planes)  # per plane: what K3 adds to the nsel counters

    def hist(self):
        G = self.G
        return np.bincount(self.wg * G.nbins + self.bin, minlength=self.nblocks * G.nbins).reshape(self.nblocks, G.nbins)

    def tile_counts(self, unit, wg):
        """Records per tile of one K3 item."""
        sel = (self.unit == unit) & (self.wg == wg)
        return np.bincount(self.tile[sel], minlength=self.G.tiles_per_unit)

    # K2 k_scan_blocks
    def scan_groups(self):
        return cdiv(self.G.nbins, SCAN_BINS)

    def scan_rows_per_lane(self):
        """`per` of k_scan_blocks: rows of the histogram one lane sums; above SCAN_KEEP they are read twice."""
        return cdiv(self.nblocks, SCAN_SEGS)

    def scan_idle_segments(self):
        """Segments of k_scan_blocks that start past the last K1 workgroup."""
        per = self.scan_rows_per_lane()
        return sum(1 for seg in range(SCAN_SEGS) if seg * per >= self.nblocks)

    # K3 k_bin_scatter
    def k3_items(self):
        return self.G.n_units * 8 * cdiv(self.nblocks, 8)

    def k3_workgroups(self, num_cus, k3_per_cu):
        return min(self.k3_items(), max(8, num_cus * max(1, k3_per_cu) // 8 * 8))

    def k3_item(self, item):
        """(unit, K1 workgroup) of a work item; the workgroup may lie past nblocks (the item is skipped)."""
        per_unit = 8 * cdiv(self.nblocks, 8)
        u = item % per_unit
        return item // per_unit, (u & 7) * (per_unit // 8) + (u >> 3)

    def k3_single(self, unit, wg):
        """The item takes its per-tile counts from K1's histogram row instead of a counting pass."""
        return self.count[unit, wg] <= SORT_BATCH and (unit * self.G.tiles_per_unit) % 2 == 0

    def k3_scan_tiles_per_lane(self):
        return cdiv(self.G.tiles_per_unit, SORT_BLOCK)

    # K3' k_sort2 (self.G is then the geometry sort2_geom returned)
    def sort2_groups(self):
        return cdiv(self.nblocks * SUB_BATCHES, SORT2_SLOTS)

    def sort2_item_totals(self):
        """item_tot[group][unit]: the records of a unit that a group of SORT2_BLOCKS K1 workgroups emitted."""
        ng = self.sort2_groups()
        return np.bincount((self.wg // SORT2_BLOCKS) * self.G.n_units + self.unit,
                           minlength=ng * self.G.n_units).reshape(ng, self.G.n_units)

    def sort2_workgroups(self, num_cus, k3_per_cu):
        nitems = self.G.n_units * self.sort2_groups()
        return min(nitems, max(8, num_cus * max(1, k3_per_cu), cdiv(nitems, S2_MAX_MINE)))

    def sort2_qualifies(self):
        return self.sort2_groups() <= MAX_SORT_GROUPS


def sub_batches(count):
    """Sizes of the sub-batches k_bin_scatter cuts an item of `count` records into."""
    count = int(count)
    return [min(SORT_BATCH, count - s0) for s0 in range(0, count, SORT_BATCH)]


def staging_rounds(nsub):
    return cdiv(int(nsub), SORT_STAGE)
