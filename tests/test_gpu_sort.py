"""The scan and sort kernels of the binned path (k_scan_blocks, k_bin_scatter, k_sort2 of slicer_sort.hip) at their
branch edges, through the C ABI.  Needs an MI355X.

Observables, all exact and all from the oracle at test time (Expect / run / check of test_gpu_project_bin_fast):
  TSC, FIXED64   accumulator words == sum rint(c 2^e) over the oracle's (xs, ys, m): a record in the wrong run, lost,
                 doubled or stored with a neighbour's mass changes a word (mass cases give every particle its own mass);
  NGP            maps and per-type maps == the oracle's, bit for bit;
  nsel           per plane and type == the oracle's count (K3 derives it from the bin bases);
  algo mask      binned alone, the project+bin kernel the case intends, bit 7 exactly when the two-level sort runs.
Every case forces the whole geometry through the handle's options (tile_log2, tile_h_log2, bin_batch, unit_rows,
k3_per_cu, k1_general, sort2), restates it with tests/sort_np.py, and asserts BEFORE the GPU is called -- as a plain
statement about the restated counts per (unit, K1 workgroup) -- that the branch it exists for is reached.  A case whose
precondition does not hold fails; none skips or shrinks.
"""
import functools

import numpy as np
import pytest

import np_restatement as npr
import oracle
import slicer_amd
import sort_np as snp
import test_gpu_project_bin_fast as pf
import test_gpu_tile_deposit as tdep
import tile_np as tnp
from slicer_amd import synth

pytestmark = pytest.mark.gpu

BOX, FOV, RND = tdep.BOX, tdep.FOV, tdep.RND  # (a centre of f32 values: the fast project+bin kernel qualifies)
ONE, THREE, FOUR = [3.0, 4.0], [3.0, 3.3, 3.6, 4.0], pf.SLABS4
SORT2 = 1 << 7


@pytest.fixture(scope="module")
def S0():
    s = slicer_amd.Slicer(0, max_chunk=1 << 20)  # (a deposit call of up to 2^20 particles is one run of K1 .. K3)
    yield s
    s.close()


@pytest.fixture
def S(S0):
    """The module's handle; every option a test sets is put back afterwards."""
    saved = {k: S0.get_option(k) for k in pf.OPTION_KEYS}
    yield S0
    try:
        S0.set_option("k4_int", saved["k4_int"])
    except slicer_amd.api.SlicerError:  # a test that failed in mid-pass left deposits in flight: a new pass drops them
        S0.plane_begin(8, 1.0, [0.0], [1.0])
    for k, v in saved.items():
        S0.set_option(k, v)


# An MI355X has 256 compute units (fewer per device in its partitioned modes), and a launch of either sort has at most
# k3_per_cu workgroups per unit: with k3_per_cu = 1 no launch has more than this many workgroups.
MAX_CUS = 256


# ---- inputs, the restatement, the GPU run -------------------------------------------------------------------------
def make_pass(npix, edges, fov=FOV, nrep=0):
    return pf.make_pass(npix, fov, RND, edges=edges, nrep=nrep)


def place(ps, plane, n, box_px, rng):
    """tdep.place for plane `plane` of a pass of several: exactly n raw positions that the oracle selects in that
    plane with (xs, ys) * npix inside the pixel rectangle box_px = (x_lo, x_hi, y_lo, y_hi)."""
    lo, hi = ps.slabs[plane]
    x_lo, x_hi, y_lo, y_hi = box_px
    out, have = [], 0
    for _ in range(8):
        m = int((n - have) * 1.3) + 2048
        cx, cy = rng.uniform(x_lo, x_hi, m) / ps.npix, rng.uniform(y_lo, y_hi, m) / ps.npix
        raw = tnp.raw_positions(cx, cy, rng.uniform(lo + 0.01, hi - 0.01, m), ps.box, ps.rnd, ps.fov)
        x, y, z = oracle.transform(raw, ps.box, ps.rnd["sgn"], ps.rnd["face"], ps.rnd["center"], ps.rnd["rcase"])
        xs, ys, _, idx = oracle.select_project(x, y, z, None, 1.0, lo, hi, ps.box, 0, ps.fov, ps.npix, want_index=True)
        px, py = xs.astype(np.float64) * ps.npix, ys.astype(np.float64) * ps.npix
        ok = (px >= x_lo) & (px < x_hi) & (py >= y_lo) & (py < y_hi)
        out.append(raw[idx[ok]])
        have += int(ok.sum())
        if have >= n:
            return np.concatenate(out)[:n]
    raise AssertionError("could not place the records")


def geom_of(ps, opts):
    return snp.geom(ps.npix, len(ps.slabs), opts["tile_log2"], opts["tile_h_log2"], opts["bin_batch"],
                    opts.get("unit_rows", 0), ps.nrep)


def chunk_of(ex, G, ngp, first=0, end=None):
    """The restated hand-off of the deposit call ex.pos[first:end] under geometry G."""
    end = len(ex.pos) if end is None else end
    entries = []
    for xs, ys, _, idx in ex.entries:
        sel = (idx >= first) & (idx < end)
        entries.append((xs[sel], ys[sel], idx[sel] - first))
    return snp.Chunk(G, entries, end - first, ngp)


def species(ps, pos, seed):
    """The same positions as a constant-mass species and with a distinct mass per particle."""
    return pf.Expect(ps, pos), pf.Expect(ps, pos, pf.exact_masses(len(pos), np.random.default_rng(seed)))


def gpu(S, ex, ngp, opts, fast=True, sort2=False, chunks=None, tag=""):
    out, mask = pf.run(S, ex, ngp=ngp, chunks=chunks, **opts)
    assert bool(mask & SORT2) == sort2, f"{tag}: two-level sort {'did not run' if sort2 else 'ran'}: mask {mask:#x}"
    return pf.check(ex, out, mask, ngp=ngp, fast=fast, sort2=sort2, tag=tag)


def three_ways(S, const, hydro, opts, fast=True, tag=""):
    """Constant mass TSC, NGP, per-particle masses TSC."""
    for ex, ngp, name in ((const, False, "tsc"), (const, True, "ngp"), (hydro, False, "tsc+mass")):
        gpu(S, ex, ngp, opts, fast=fast, tag=f"{tag} {name}")


# ---- 1. sub-batches and staging rounds ------------------------------------------------------------------------------
OPTS_256 = dict(tile_log2=5, tile_h_log2=5, bin_batch=32768)  # 8 x 8 tiles of 32 x 32 pixels, one K1 workgroup


@functools.lru_cache(maxsize=None)
def spread_positions(n):
    return tdep.place(n, 256, (0.5, 255.5, 0.5, 255.5), np.random.default_rng(n))


# count -> (sub-batches, staging rounds of the last one, counts from K1's histogram row)
SUBS = {30000: ([8192, 8192, 8192, 5424], 2, False), 8192: ([8192], 2, True), 8193: ([8192, 1], 1, False),
        4096: ([4096], 1, True), 4097: ([4097], 2, True), 12288: ([8192, 4096], 1, False),
        12289: ([8192, 4097], 2, False)}


@pytest.mark.parametrize("general", [0, 1], ids=["fast", "general"])
@pytest.mark.parametrize("n", list(SUBS))
def test_sub_batches_and_staging_rounds(S, n, general):
    """One item of n records (one plane, one K1 workgroup, every particle selected and on the map): k_bin_scatter's
    `for s0 < count; s0 += kSortBatch` with the cursor carry `cur[i] += pos[i]` and a ragged last sub-batch, its
    `for lo < nsub; lo += kSortStage` with one and two rounds, `single` on both sides of count <= kSortBatch."""
    ps = make_pass(256, ONE)
    const, hydro = species(ps, spread_positions(n), n)
    G = geom_of(ps, OPTS_256)
    subs, rounds, single = SUBS[n]
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        assert c.nblocks == 1 and c.count.tolist() == [[n]] and G.n_units == 1
        assert snp.sub_batches(c.count[0, 0]) == subs and all(s == snp.SORT_BATCH for s in subs[:-1])
        assert snp.staging_rounds(subs[-1]) == rounds and (subs[-1] > snp.SORT_STAGE) == (rounds == 2)
        assert c.k3_single(0, 0) == single == (n <= snp.SORT_BATCH)
    three_ways(S, const, hydro, dict(OPTS_256, k1_general=general), fast=not general, tag=f"n {n}")


# ---- 2. a whole sub-batch in one tile ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_tile_positions(tile, single):
    rng = np.random.default_rng(tile + 100 * single)
    def inside(t, n):
        x0, y0 = 32 * (t % 8), 32 * (t // 8)
        return tdep.place(n, 256, (x0 + 0.5, x0 + 31.5, y0 + 0.5, y0 + 31.5), rng)
    n_tile = (1 if single else 3) * snp.SORT_BATCH - 2
    body = inside(tile, n_tile)
    cut = n_tile // 3
    return np.concatenate([body[:cut], inside(tile - 1, 1), body[cut:], inside(tile + 1, 1)])


@pytest.mark.parametrize("single", [True, False], ids=["histogram-row", "counting-pass"])
@pytest.mark.parametrize("tile", [27, 28], ids=["odd-tile", "even-tile"])
def test_a_whole_sub_batch_in_one_tile(S, tile, single):
    """All but two records of an item in one tile, one record in each neighbour: a packed u16 count of up to
    kSortBatch in the upper (odd tile) or lower (even tile) half of its word next to a neighbour's count of 1, in
    `cnt[i] = hrow[i]` / the LDS `atomicAdd(&cnt[tile >> 1], 1u << 16 (tile & 1))` and in get16 of the scan.  With
    three sub-batches and two records outside the tile, at least one sub-batch of kSortBatch lies in the tile whole."""
    ps = make_pass(256, ONE)
    const, hydro = species(ps, one_tile_positions(tile, single), tile)
    G = geom_of(ps, OPTS_256)
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        per_tile = c.tile_counts(0, 0)
        subs = snp.sub_batches(c.count[0, 0])
        assert c.nblocks == 1 and subs == [snp.SORT_BATCH] * (1 if single else 3)
        assert per_tile[tile - 1] == 1 and per_tile[tile + 1] == 1 and per_tile[tile] == c.count[0, 0] - 2
        assert c.k3_single(0, 0) == single and (single or c.count[0, 0] - per_tile[tile] < len(subs))
    three_ways(S, const, hydro, OPTS_256, tag=f"tile {tile} single {single}")


# ---- 3. an odd tile count ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd_positions():
    ps = make_pass(48, THREE)
    rng = np.random.default_rng(3)
    pos = np.concatenate([place(ps, p, 1500, (0.5, 47.5, 0.5, 47.5), rng) for p in range(3)])
    return pos[rng.permutation(len(pos))]


def test_odd_tile_count(S):
    """Three planes of 3 x 3 tiles (48^2, 16 x 16): units 0 and 2 start on an even bin and take `single`, where the
    last word of K1's histogram row also holds the next unit's first tile and `hrow[i] & 0xFFFF` is all that keeps it
    out; unit 1 starts on bin 9, `(plane * tpp) & 1`, and takes the counting pass with a count below kSortBatch.
    k_scan_blocks runs with an odd nbins (stride16 = nbins + 1), one partial group and 31 idle segments."""
    ps = make_pass(48, THREE)
    opts = dict(tile_log2=4, tile_h_log2=4, bin_batch=32768)
    const, hydro = species(ps, odd_positions(), 3)
    G = geom_of(ps, opts)
    assert G.tiles_per_unit == 9 and G.n_units == 3 and G.nbins == 27 and G.nbins % 2 == 1 and G.nbins % snp.SCAN_BINS
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        assert c.nblocks == 1 and c.scan_groups() == 1 and c.scan_idle_segments() == snp.SCAN_SEGS - 1
        assert c.k3_single(0, 0) and c.k3_single(2, 0) and not c.k3_single(1, 0)
        assert 0 < c.count[1, 0] <= snp.SORT_BATCH and (1 * G.tiles_per_unit) % 2 == 1
        # the u16 next to unit 0's (unit 2's would-be) last count is not empty
        assert c.tile_counts(0, 0)[8] > 0 and c.tile_counts(1, 0)[0] > 0 and c.tile_counts(2, 0)[8] > 0
    three_ways(S, const, hydro, opts, tag="odd")


# ---- 4. wide units, many scan groups, bands ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_positions():
    """520^2, four planes: a spread of records plus the first and the last tile column filled from top to bottom, so
    that the first and last tile of every band is occupied whatever the band height."""
    ps = make_pass(520, FOUR)
    rng = np.random.default_rng(4)
    parts = []
    for p in range(4):
        parts += [place(ps, p, 4000, (0.5, 519.5, 0.5, 519.5), rng), place(ps, p, 1500, (0.5, 7.5, 0.5, 519.5), rng),
                  place(ps, p, 1500, (512.5, 519.5, 0.5, 519.5), rng),
                  place(ps, p, 60, (488.5, 519.5, 512.5, 519.5), rng)]  # the last four tiles of the map
    pos = np.concatenate(parts)
    return pos[rng.permutation(len(pos))]


WIDE = dict(tile_log2=3, tile_h_log2=3, bin_batch=32768)


@pytest.mark.parametrize("unit_rows", [0, 13], ids=["bands31", "bands13"])
def test_wide_units_and_many_scan_groups(S, unit_rows):
    """65 x 65 tiles of 8 x 8 pixels, four planes: choose_geom cuts the planes into bands.  `per` of k_bin_scatter's
    scan is 4 (2015 tiles per unit) / 2 (845), tiles_per_unit is odd, nbins > 16384 fills the second slot of the
    kPerLane = 2 group-sum scan, the last scan group is partial.  With bands of 31 rows the last band of a plane has 3
    rows and 1820 bins that stay empty (the scan groups behind the last used bin sum to 0); with bands of 13 rows every
    bin is in use and the partial last group holds records."""
    ps = make_pass(520, FOUR)
    opts = dict(WIDE, unit_rows=unit_rows)
    const, hydro = species(ps, wide_positions(), 4)
    G = geom_of(ps, opts)
    assert G.units_per_plane == (5 if unit_rows else 3) and G.tiles_per_unit == (845 if unit_rows else 2015)
    assert G.tiles_per_unit > snp.SORT_BLOCK and G.tiles_per_unit % 2 == 1 and G.nbins > 16384 and G.nbins % snp.SCAN_BINS
    assert (G.rows_per_unit * G.units_per_plane > G.nty) == (unit_rows == 0)
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        assert c.nblocks == 1 and c.scan_groups() > 512 and c.k3_scan_tiles_per_lane() == (2 if unit_rows else 4)
        used = np.nonzero(np.bincount(c.bin, minlength=G.nbins))[0]
        for u in range(G.n_units):
            rows = min(G.rows_per_unit, G.nty - (u % G.units_per_plane) * G.rows_per_unit)  # tile rows the band has
            per_tile = c.tile_counts(u, 0)
            assert per_tile[0] > 0 and per_tile[rows * G.ntx - 1] > 0 and not per_tile[rows * G.ntx:].any()
            assert c.k3_single(u, 0) == (u % 2 == 0) and c.count[u, 0] <= snp.SORT_BATCH
        if unit_rows:
            assert used[-1] // snp.SCAN_BINS == c.scan_groups() - 1  # records in the partial last group
        else:
            assert used[-1] // snp.SCAN_BINS < c.scan_groups() - 1 and used[-1] // snp.SCAN_BINS >= 512
    three_ways(S, const, hydro, opts, tag=f"wide unit_rows {unit_rows}")


def test_the_widest_unit(S):
    """One plane of 128 x 64 tiles (1024^2, 8 x 16 pixels): 8192 tiles in one unit, all that choose_geom admits, so
    `per` = 16 tiles per lane in k_bin_scatter's scan and the cnt / pos / cur tables at their largest; records in the
    first and the last tile."""
    ps = make_pass(1024, ONE)
    opts = dict(tile_log2=3, tile_h_log2=4, bin_batch=32768)
    rng = np.random.default_rng(10)
    pos = np.concatenate([tdep.place(20000, 1024, (0.5, 1023.5, 0.5, 1023.5), rng),
                          tdep.place(40, 1024, (0.5, 7.5, 0.5, 15.5), rng),
                          tdep.place(40, 1024, (1016.5, 1023.5, 1008.5, 1023.5), rng)])
    const, hydro = species(ps, pos[rng.permutation(len(pos))], 10)
    G = geom_of(ps, opts)
    assert G.units_per_plane == 1 and G.tiles_per_unit == 8192 == G.nbins and G.n_units == 1
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        per_tile = c.tile_counts(0, 0)
        assert c.nblocks == 1 and c.k3_scan_tiles_per_lane() == 16 and per_tile[0] >= 40 and per_tile[8191] >= 40
        assert len(snp.sub_batches(c.count[0, 0])) == 3 and c.scan_groups() == 256
    three_ways(S, const, hydro, opts, tag="8192 tiles")


def test_thin_bands_on_a_small_map(S):
    """96^2, four planes, 6 x 6 tiles, unit_rows = 4: two bands per plane, the second two rows high.  `bin0`, the
    `lrow` / `row` offsets and workgroup 0's per-plane counters `at((p + 1) bpp) - at(p bpp)` with
    bpp = units_per_plane * tiles_per_unit; nsel of every plane is compared by check()."""
    ps = make_pass(96, FOUR)
    opts = dict(tile_log2=4, tile_h_log2=4, bin_batch=4096, unit_rows=4)
    rng = np.random.default_rng(5)
    # (different numbers of records per plane: a counter that took another plane's bins shows)
    pos = np.concatenate([place(ps, p, 1000 + 800 * p, (0.5, 95.5, 0.5, 95.5), rng) for p in range(4)])
    const, hydro = species(ps, pos[rng.permutation(len(pos))], 5)
    G = geom_of(ps, opts)
    assert G.units_per_plane == 2 and G.rows_per_unit == 4 and G.tiles_per_unit == 24 and G.n_units == 8
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        assert c.nblocks == 3 and c.records.tolist() == [1000, 1800, 2600, 3400] and (c.count > 0).all()
        for u in range(8):
            assert not c.tile_counts(u, 0)[12:].any() if u % 2 else c.tile_counts(u, 0)[23] > 0
    three_ways(S, const, hydro, opts, tag="thin bands")


# ---- 5. persistent workgroups -----------------------------------------------------------------------------------------
def test_persistent_workgroups_take_several_items(S):
    """k3_per_cu = 1, 32 units (four planes of eight one-row bands), 19 K1 workgroups of 1024 particles: 768 items
    for the launch's workgroups, so `item += gridDim.x` runs on with the cnt / pos / cur tables of the item before;
    items with `count == 0` (K1 workgroup 3 sends everything to unit 0) and with `lb >= nblocks` (19 is no multiple
    of 8) are passed over.  Per-particle masses: a stale table moves a record to another particle's place."""
    ps = make_pass(128, FOUR)
    opts = dict(tile_log2=4, tile_h_log2=4, bin_batch=1024, unit_rows=1, k3_per_cu=1)
    rng = np.random.default_rng(6)
    n = 18 * 1024 + 300
    pos = np.concatenate([place(ps, p, n // 4, (0.5, 127.5, 0.5, 127.5), rng) for p in range(4)])
    pos = pos[rng.permutation(n)]
    pos[3 * 1024:4 * 1024] = place(ps, 0, 1024, (0.5, 127.5, 0.5, 15.5), rng)
    const, hydro = species(ps, pos, 6)
    G = geom_of(ps, opts)
    assert G.n_units == 32 and G.tiles_per_unit == 8 and G.batch == 1024
    for ngp in (False, True):
        c = chunk_of(hydro, G, ngp)
        nwg = c.k3_workgroups(MAX_CUS, 1)
        assert c.nblocks == 19 and c.nblocks % 8 and c.k3_items() == 768 > 2 * nwg and nwg == MAX_CUS
        items = [c.k3_item(i) for i in range(c.k3_items())]
        assert sum(1 for _, w in items if w >= c.nblocks) == 32 * 5
        assert c.count[0, 3] == 1024 and not c.count[1:, 3].any() and (c.count == 0).sum() >= 31
        # more items with records than the largest launch has workgroups: some workgroup sorts a second item with the
        # tables of its first, whatever the number of workgroups; items without records lie between them
        live = np.array([w < c.nblocks and c.count[u, w] > 0 for u, w in items])
        assert live.sum() > 2 * nwg and (~live[:live.nonzero()[0][-1]]).sum() >= 31 + 32 * 4
    gpu(S, hydro, False, opts, tag="persistent tsc+mass")
    gpu(S, hydro, True, opts, tag="persistent ngp+mass")
    gpu(S, const, False, opts, tag="persistent tsc")


# ---- 6. long scan columns -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case():
    ps = make_pass(256, ONE)
    return pf.Expect(ps, synth.positions(0, 513 * 1024 + 100, BOX))


@pytest.mark.parametrize("bin_batch", [1024, 32768], ids=["514-workgroups", "17-workgroups"])
def test_long_and_short_scan_columns(S, bin_batch):
    """One deposit call of 525412 particles.  bin_batch = 1024: 514 K1 workgroups, `per` = 17 > kKeep in
    k_scan_blocks, so `kept` is false and hist16 is read a second time for the prefixes.  bin_batch = 32768: 17
    workgroups, `kept` with one row per lane and 15 segments whose `lo` lies past nblocks."""
    ex = long_case()
    opts = dict(OPTS_256, bin_batch=bin_batch)
    G = geom_of(ex.ps, opts)
    for ngp in (False, True):
        c = chunk_of(ex, G, ngp)
        if bin_batch == 1024:
            assert c.nblocks == 514 > 512 and c.scan_rows_per_lane() == 17 > snp.SCAN_KEEP and c.scan_idle_segments() == 1
        else:
            assert c.nblocks == 17 < snp.SCAN_SEGS and c.scan_rows_per_lane() == 1 and c.scan_idle_segments() == 15
        assert (c.count > 0).all() and c.count.sum() > 300000
    gpu(S, ex, True, opts, tag=f"bin_batch {bin_batch} ngp")
    gpu(S, ex, False, opts, tag=f"bin_batch {bin_batch} tsc")


# ---- 7. regions larger than the batch -----------------------------------------------------------------------------------
def test_replication_regions(S):
    """nrepperp = 1 on a 64^2 map: nine replicas per particle, the batch is cut to 65535 / 9 rounded down to 1024s and
    a (unit, K1 workgroup) region is nine batches long (`r0 = (plane nblocks + lb) region`); the general project+bin
    kernel feeds items of several sub-batches."""
    ps = make_pass(64, ONE, fov=0.5, nrep=1)
    opts = dict(tile_log2=4, tile_h_log2=4, bin_batch=32768)
    const, hydro = species(ps, synth.positions(0, 7168 + 3000, BOX), 7)
    G = geom_of(ps, opts)
    assert G.reps == 9 and G.batch == 7168 and G.region == 9 * G.batch
    for ngp in (False, True):
        c = chunk_of(const, G, ngp)
        assert c.nblocks == 2 and c.count[0, 0] > 2 * snp.SORT_BATCH and c.count[0, 0] > 2 * G.batch and c.count[0, 1] > 0
    gpu(S, const, True, opts, fast=False, tag="nrep ngp")
    gpu(S, hydro, False, opts, fast=False, tag="nrep tsc+mass")
    gpu(S, const, False, opts, fast=False, tag="nrep tsc")


# ---- 8. the two-level sort ------------------------------------------------------------------------------------------------
def sort2_both(S, ex, opts, tag):
    opts = dict(opts, sort2=1, k1_stack=0)
    gpu(S, ex, False, opts, sort2=True, tag=f"{tag} tsc")
    gpu(S, ex, True, opts, sort2=True, tag=f"{tag} ngp")


def sort2_chunk(ex, opts, ngp):
    G2 = snp.sort2_geom(geom_of(ex.ps, opts))
    assert G2 is not None, "the pass does not fit the two-level sort"
    c = chunk_of(ex, G2, ngp)
    assert c.sort2_qualifies()
    return G2, c


def test_sort2_items_of_several_windows(S):
    """One plane of 8 x 8 tiles: the units of the two-level sort are the 8 tile rows.  20000 records of one K1
    workgroup in tile row 3 make an item of more than kS2Cap records: `multi`, the counting pass, then three windows
    with `cur[]` carried, the last one ragged."""
    ps = make_pass(256, ONE)
    rng = np.random.default_rng(8)
    pos = np.concatenate([tdep.place(20000, 256, (0.5, 255.5, 96.5, 127.5), rng), spread_positions(4097)[:3000]])
    ex = pf.Expect(ps, pos[rng.permutation(len(pos))])
    for ngp in (False, True):
        G2, c = sort2_chunk(ex, OPTS_256, ngp)
        tot = c.sort2_item_totals()
        assert G2.n_units == 8 and G2.tiles_per_unit == 8 and tot.shape == (1, 8)
        assert 2 * snp.S2_CAP < tot[0, 3] < 3 * snp.S2_CAP and tot[0, 3] % snp.S2_CAP and (tot > 0).all()
        assert tot[0].max() == tot[0, 3] and np.sort(tot[0])[-2] <= snp.S2_CAP  # the other items take one window
    sort2_both(S, ex, OPTS_256, "sort2 multi")


@functools.lru_cache(maxsize=None)
def four_plane_case(npix, n):
    return pf.Expect(make_pass(npix, FOUR), synth.positions(0, n, BOX))


@pytest.mark.parametrize("npix,units,tiles", [(128, 64, 16), (520, 132, 130), (512, 64, 256)],
                         ids=["64-units", "132-units", "256-tiles"])
def test_sort2_unit_and_tile_limits(S, npix, units, tiles):
    """Four planes of 8 x 8-pixel tiles.  128^2: exactly 64 units of one tile row (K1's stage_flush takes its
    `nu <= 64` side with every lane a unit, the table row of 64 starts + the end).  520^2: 132 units of two rows
    (`nu > 64`, the shared prefix table).  512^2: 64 units of four rows = 256 tiles, the 8-bit limit of scol[]."""
    if npix == 520:
        ex = pf.Expect(make_pass(520, FOUR), wide_positions())
    else:
        ex = four_plane_case(npix, 40000)
    opts = dict(tile_log2=3, tile_h_log2=3, bin_batch=4096)
    for ngp in (False, True):
        G2, c = sort2_chunk(ex, opts, ngp)
        tot = c.sort2_item_totals()
        assert G2.n_units == units and G2.tiles_per_unit == tiles and G2.n_units <= snp.MAX_COARSE
        assert (tot.sum(axis=0) > 0).all() and c.nblocks > 1  # every unit has records
        assert np.bincount(c.tile, minlength=tiles)[[0, tiles - 1]].all()  # the first and the last tile id occur
    sort2_both(S, ex, opts, f"sort2 {units} units")


def test_sort2_workgroups_take_several_items(S):
    """64 units x 6 groups of 16 K1 workgroups (bin_batch = 1024, 81 workgroups) with k3_per_cu = 1: more items than
    the launch has workgroups, so `it += gridDim.x` runs on and s_mybase[] holds several bases per workgroup."""
    ex = four_plane_case(128, 80 * 1024 + 500)
    opts = dict(tile_log2=3, tile_h_log2=3, bin_batch=1024, k3_per_cu=1)
    for ngp in (False, True):
        G2, c = sort2_chunk(ex, opts, ngp)
        tot = c.sort2_item_totals()
        assert c.nblocks == 81 and c.sort2_groups() == 6 and G2.n_units == 64
        nwg = c.sort2_workgroups(MAX_CUS, 1)
        # item it = group * n_units + unit; more items with records than the largest launch has workgroups
        assert tot.size == 384 > nwg == MAX_CUS and (tot > 0).sum() > nwg
    sort2_both(S, ex, opts, "sort2 items")


# ---- the largest mass K3 hands to the tile deposit ----------------------------------------------------------------------
def test_two_species_and_the_mass_maximum(S):
    """Two species with per-particle masses three decades apart in one pass with one shared accumulator, the light one
    first (the pattern of test_hydro_two_species_share_one_integer_cell_quantum): k_bin_scatter's mass_max reduction
    over all sub-batches (30000 and 9000 records: four and two, the last ones ragged) feeds T.max_mass, from which the
    tile deposit takes the quantum 2^(le - 49) of its integer cells.
      FIXED64: accumulator == sum rint(c 2^30) over both species, bit for bit.
      F32 with integer cells: a pixel that one work item alone reaches (J = 1) with all its contributions multiples of
      the quantum and a sum below 2^53 quanta is flushed by one conversion `(float)((double)cell * 2^(le - 49))` into
      a zero map cell: it equals RN32 of the exact sum.  A maximum that misses the heavy species puts its
      contributions beyond the 2^52 window of the integer conversion."""
    ps = make_pass(256, ONE)
    rng = np.random.default_rng(9)
    n_l, n_h = 30000, 9000
    pos = [spread_positions(30000), spread_positions(12289)[:n_h]]
    m_l = pf.exact_masses(n_l, rng)
    m_h = (pf.exact_masses(n_h, rng).astype(np.float64) * 4096.0).astype(np.float32)
    m_h[m_h > 1000.0] = 2000.0
    sp = [pf.Expect(ps, pos[0], m_l), pf.Expect(ps, pos[1], m_h)]
    types = (0, 4)
    G = geom_of(ps, OPTS_256)
    for ex, n in zip(sp, (n_l, n_h)):
        c = chunk_of(ex, G, False)
        assert c.count.tolist() == [[n]] and len(snp.sub_batches(n)) == (4 if n == n_l else 2) and n % snp.SORT_BATCH
    xs, ys, ms = (np.concatenate([ex.entries[0][k] for ex in sp]) for k in range(3))
    ms = tnp.cap_mass(ms)
    top = [float(tnp.cap_mass(ex.entries[0][2]).max()) for ex in sp]
    le = tnp.mass_le(max(top))
    assert top[1] > 500 * top[0] and le == tnp.mass_le(top[1]) >= tnp.mass_le(top[0]) + 9
    pix, val = npr.tsc_contributions(xs, ys, ms, ps.npix)
    P = tnp.Pixels(pix, val, ps.npix, le)
    gx, gy = snp.centre_cells(xs, ys, ps.npix)
    _, tile = snp.cell_to_tile(gx, gy, 0, G)
    J, parts = tnp.addends(P, pix, val, tile, np.zeros(len(xs), np.int64), True)
    E = P.exact()
    assert max(parts.values()) == 1  # every bin is one work item
    quantum_ok = P.count(tnp.not_quantum(P.v.astype(np.float32), le)) == 0
    lone = (J == 1) & quantum_ok & np.array([e >> 111 < 1 << 53 for e in E])
    heavy_px = np.zeros(ps.npix * ps.npix, bool)
    heavy_px[pix[len(sp[0].entries[0][0]):][pix[len(sp[0].entries[0][0]):] >= 0]] = True
    assert lone.sum() > 20000 and heavy_px[P.upix[lone]].sum() > 5000

    def one_pass(accum, k4_int):
        for k, v in dict(OPTS_256, k4_int=k4_int, k1_general=0, k1_stack=-1, sort2=0, unit_rows=0).items():
            S.set_option(k, v)
        S.plane_begin(ps.npix, ps.fov, [3.0], [4.0], mas=slicer_amd.MAS_TSC, accum=accum, algo=slicer_amd.ALGO_BINNED,
                      hydro=True, want_type_maps=False)
        npart = [0] * 6
        npart[types[0]], npart[types[1]] = n_l, n_h
        S.file_begin(npart, [0.0] * 6, BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
        for t, ex in zip(types, sp):
            S.deposit_host(t, ex.pos, ex.mass)
        S.file_end()
        acc = None
        if accum == pf.FIXA:
            S.plane_flush()
            ptrs, _ = S.plane_accumulators(0)
            acc = S.to_host(ptrs[6], (ps.npix, ps.npix), np.uint64)
        tot, _, nsel = S.plane_read(0, want_types=False)
        mask = S.algo_mask()
        assert (mask & 7) == 1 << slicer_amd.ALGO_BINNED and mask & pf.FAST and not mask & (pf.GENERAL | SORT2), hex(mask)
        assert [int(nsel[t]) for t in types] == [n_l, n_h] and int(nsel.sum()) == n_l + n_h
        return tot, acc, mask

    tot, acc, mask = one_pass(pf.FIXA, 2)
    want = P.full(P.fixed(30), np.int64)
    assert np.array_equal(acc.view(np.int64), want), f"{np.count_nonzero(acc.view(np.int64) != want)} accumulator words differ"
    tot, _, mask = one_pass(pf.F32A, 2)
    assert mask & (1 << 6), f"integer cells did not run: mask {mask:#x}"
    want32 = np.array([tnp._rn32(int(e), le - 160) for e in E[lone]], np.float32)
    got32 = tot.reshape(-1)[P.upix[lone]]
    bad = np.nonzero(got32.view(np.uint32) != want32.view(np.uint32))[0]
    assert len(bad) == 0, f"{len(bad)} of {lone.sum()} single-addend pixels differ from RN32 of the exact sum"
