"""The LDS tile deposit (k_build_items, k_tile_deposit) against exact per-pixel sums, through the C ABI.  Needs an MI355X.

Reference: np_restatement.tsc_contributions on the oracle's transform / select_project output (bit-exact per
contribution), summed exactly per pixel in integers (tests/tile_np.py) -- E.  Asserted contracts, all
derived, none measured, compared in integer arithmetic:
  FIXED64   accumulator == sum rint(c 2^e) bit for bit, map == RN32 of it; e = 40 - (ilogb(m) + 1), 30 with masses.
  F64       |acc - E| <= 2J 2^-53 E, map == RN32(acc); with f64 cells forced (k4_int = 0) the tile sum itself is a
            sequential f64 sum of the k contributions, so k 2^-53 E is added as in the F32 mode.
  F32       |map - E| <= (2J - 1) 2^-24 E, plus k 2^-53 E with f64 cells; a pixel with one contribution is exact.
J (tile_np.addends) is restated from the forced tile geometry, the chunks per launch and the part rule of
k_build_items, including its lower whole-bin cap in launches with integer cells.
Every input condition -- records per bin, predicted noted records, k >> J -- is asserted before the GPU is called.
Per-particle masses that are NaN or negative (tests/test_gpu_hostile_particles.py): E, k and J come from the other
entries (clean_mass), the NaN pixels of an F32 / F64 map must be exactly the oracle's (Case.nan_mask) and are left out
of the value comparison; a FIXED64 map holds no NaN.  With ALGO_DIRECT every contribution is an atomic add of its own:
J = k.
"""
import functools

import numpy as np
import pytest

import np_restatement as npr
import oracle
import slicer_amd
import tile_np as tnp
from slicer_amd import synth

pytestmark = pytest.mark.gpu

BOX, FOV, LD, LD2 = 1000.0, 0.25, 3.0, 4.0
# (a centre of f32 values: the fast project+bin kernel, and with it the two-level sort, qualify)
RND = dict(sgn=(-1, 1, -1), face=3, center=(0.3125, 0.625, 0.125), rcase=3.0)
F32A, F64A, FIXA = slicer_amd.ACC_F32, slicer_amd.ACC_F64, slicer_amd.ACC_FIXED64
ACC_IDS = {F32A: "F32", F64A: "F64", FIXA: "FIXED64"}
OPTION_KEYS = ("k4_int", "tile_log2", "tile_h_log2", "sort2", "pending", "k1_stack")
M_CONST = 0.0123


@pytest.fixture(scope="module")
def S0():
    s = slicer_amd.Slicer(0, max_chunk=1 << 20)
    yield s
    s.close()


@pytest.fixture
def S(S0):
    """The module's handle; every option a test sets is put back afterwards."""
    saved = {k: S0.get_option(k) for k in OPTION_KEYS}
    yield S0
    try:
        S0.set_option("k4_int", saved["k4_int"])
    except slicer_amd.api.SlicerError:  # a test that failed in mid-pass left deposits in flight: a new pass drops them
        S0.plane_begin(8, 1.0, [0.0], [1.0])
    for k, v in saved.items():
        S0.set_option(k, v)


# ---- inputs -----------------------------------------------------------------------------------------------------
def forward(pos, mass, mconst, npix):
    """The oracle's projection of raw positions: xs, ys, capped masses, particle index of every selected record."""
    x, y, z = oracle.transform(pos, BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
    xs, ys, ms, idx = oracle.select_project(x, y, z, mass, mconst, LD, LD2, BOX, 0, FOV, npix, want_index=True)
    return xs, ys, tnp.cap_mass(ms), idx


def centre_pixels(xs, ys, npix):
    dl = 1.0 / np.float64(npix)
    return np.floor(xs.astype(np.float64) / dl).astype(np.int64), np.floor(ys.astype(np.float64) / dl).astype(np.int64)


def place(n, npix, box_px, rng, keep=None, reject=None):
    """Exactly n raw positions whose oracle projection has its centre pixel / offsets as asked: candidates are drawn in
    the pixel rectangle box_px = (x_lo, x_hi, y_lo, y_hi) (pixel units), projected with the oracle, and kept by
    `keep(xs, ys, gx, gy)` (default: inside the rectangle), minus `reject`."""
    x_lo, x_hi, y_lo, y_hi = box_px
    out, have = [], 0
    for _ in range(8):
        m = int((n - have) * 1.3) + 4096
        cx, cy = rng.uniform(x_lo, x_hi, m) / npix, rng.uniform(y_lo, y_hi, m) / npix
        raw = tnp.raw_positions(cx, cy, rng.uniform(3.05, 3.95, m), BOX, RND, FOV)
        xs, ys, _, idx = forward(raw, None, 1.0, npix)
        gx, gy = centre_pixels(xs, ys, npix)
        if keep is None:
            px, py = xs.astype(np.float64) * npix, ys.astype(np.float64) * npix
            ok = (px >= x_lo) & (px < x_hi) & (py >= y_lo) & (py < y_hi)
        else:
            ok = keep(xs, ys, gx, gy)
        if reject is not None:
            ok &= ~reject(xs, ys, gx, gy)
        out.append(raw[idx[ok]])
        have += int(ok.sum())
        if have >= n:
            return np.concatenate(out)[:n]
    raise AssertionError("could not place the records")


def decade_masses(n, rng, top=2e-5):
    """Per-particle masses over four decades below `top`, ~1 % above MAX_M (they count as 0) and ~1 % exactly 0."""
    m = (top * 10.0 ** rng.uniform(-4, 0, n)).astype(np.float32)
    m[rng.random(n) < 0.01] = 2000.0
    m[rng.random(n) < 0.01] = 0.0
    m[::50] = np.float32(top)  # (every chunk sees the largest mass: one quantum for all launches of a pass)
    return m


def clean_mass(ms):
    """Capped masses with the entries that poison a TSC map (NaN or negative: the root is NaN) set to 0 -> masses, and
    which entries those were."""
    ms = np.asarray(ms, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(ms) & (ms >= 0)
    return np.where(ok, ms, np.float32(0)).astype(np.float32), ~ok


class Case:
    """Positions (and masses) of one species, cut into deposit calls; the restatement of what the design does with
    them for a tile geometry."""

    def __init__(self, npix, tl, pos, mass, mconst, files=None):
        self.npix, self.tl, self.pos, self.mass, self.mconst = npix, tl, np.ascontiguousarray(pos, np.float32), mass, mconst
        self.hydro = mass is not None
        self.ptype = 0 if self.hydro else 1
        n = len(self.pos)
        self.files = files if files is not None else [[(0, n)]]  # files -> deposit calls (first, end)
        xs, ys, ms, idx = forward(self.pos, mass, 0.0 if self.hydro else mconst, npix)
        self.nan_mask = None  # the oracle's NaN pixels (TSC), where a mass poisons its footprint
        capped = ms
        ms, poisoned = clean_mass(capped)
        if poisoned.any():
            self.nan_mask = np.isnan(oracle.gridist_w(xs, ys, capped, npix, False))
        self.xs, self.ys, self.ms, self.idx, self.poisoned = xs, ys, ms, idx, poisoned
        gx, gy = centre_pixels(xs, ys, npix)
        self.gx, self.gy = gx, gy
        ntx = (npix + (1 << tl) - 1) >> tl
        self.bin = (np.clip(gy, 0, npix - 1) >> tl) * ntx + (np.clip(gx, 0, npix - 1) >> tl)
        self.chunk = np.zeros(len(idx), np.int64)  # deposit call of every record, in order
        c = 0
        for f in self.files:
            for a, b in f:
                self.chunk[(idx >= a) & (idx < b)] = c
                c += 1
        self.nchunks = c
        self.le = tnp.mass_le(ms.max() if self.hydro else mconst)
        self.pix, self.val = npr.tsc_contributions(xs, ys, ms, npix)
        self.P = tnp.Pixels(self.pix, self.val, npix, self.le)
        self.E = self.P.exact()
        self.k = self.P.count()
        self.fixed_exp = 40 - (10 if self.hydro else tnp.mass_le(mconst))
        self.noted = tnp.noted_records(self.val, ms, self.le)

    @functools.lru_cache(maxsize=None)
    def J(self, int_cells, pending):
        return tnp.addends(self.P, self.pix, self.val, self.bin, self.chunk // pending, int_cells)

    def bin_count(self, b, launch=None, pending=32):
        sel = self.bin == b
        if launch is not None:
            sel &= (self.chunk // pending) == launch
        return int(sel.sum())


def run(S, case, accum, k4_int, sort2=0, pending=32, ngp=False, algo=slicer_amd.ALGO_BINNED):
    S.set_option("tile_log2", case.tl)
    S.set_option("tile_h_log2", case.tl)
    S.set_option("k4_int", k4_int)
    S.set_option("sort2", sort2)
    S.set_option("pending", pending)
    S.plane_begin(case.npix, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP if ngp else slicer_amd.MAS_TSC, accum=accum,
                  algo=algo, hydro=case.hydro)
    for f in case.files:
        npart, massarr = [0] * 6, [0.0] * 6
        npart[case.ptype] = sum(b - a for a, b in f)
        massarr[case.ptype] = 0.0 if case.hydro else case.mconst
        S.file_begin(npart, massarr, BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
        for a, b in f:
            S.deposit_host(case.ptype, case.pos[a:b], case.mass[a:b] if case.hydro else None)
        S.file_end()
    acc = None
    if not ngp and accum != F32A:
        S.plane_flush()
        ptrs, _ = S.plane_accumulators(0)
        acc = S.to_host(ptrs[case.ptype], (case.npix, case.npix), np.float64 if accum == F64A else np.uint64)
    tot, toti, nsel = S.plane_read(0)
    mask = S.algo_mask()  # (after the read: the pending chunks' tile launch has happened)
    assert (mask & 7) == 1 << algo, f"the {'binned' if algo == slicer_amd.ALGO_BINNED else 'direct'} path did not run alone: mask {mask:#x}"
    assert int(nsel[case.ptype]) == len(case.xs) and int(nsel.sum()) == len(case.xs)
    assert same_bits(tot, toti[case.ptype])  # one species: the sum is that map
    return tot, acc, mask


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN (payloads are not part of the contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    q = np.uint32(0x7FC00000)
    return np.array_equal(np.where(np.isnan(a), q, a.view(np.uint32)), np.where(np.isnan(b), q, b.view(np.uint32)))


def check(case, tot, acc, mask, accum, k4_int, sort2=0, pending=32, tag="", algo=slicer_amd.ALGO_BINNED):
    P, E, k = case.P, case.E, case.k
    direct = algo == slicer_amd.ALGO_DIRECT
    int_cells = k4_int == 2 and accum != FIXA and not direct
    nan = case.nan_mask if getattr(case, "nan_mask", None) is not None else np.zeros((case.npix, case.npix), bool)
    assert bool(mask & (1 << 6)) == int_cells, f"{tag}: integer cells {'did not run' if int_cells else 'ran'}: {mask:#x}"
    assert bool(mask & (1 << 7)) == bool(sort2), f"{tag}: run-table walk: mask {mask:#x}"
    touched = np.zeros(case.npix * case.npix, bool)
    touched[P.upix] = True
    assert not tot.reshape(-1)[~touched].any(), f"{tag}: mass in a pixel no contribution reaches"
    if accum == FIXA:
        assert np.isfinite(tot).all(), f"{tag}: a FIXED64 map holds a NaN or an infinity"
        want = P.full(P.fixed(case.fixed_exp), np.int64)
        bad = np.argwhere(acc.view(np.int64) != want)
        assert len(bad) == 0, f"{tag}: FIXED64 accumulator differs at {bad[:4]} of {len(bad)} pixels"
        want32 = (want.astype(np.float32) * np.float32(np.ldexp(1.0, -case.fixed_exp))).astype(np.float32)
        assert np.array_equal(tot.view(np.uint32), want32.view(np.uint32)), f"{tag}: FIXED64 map != RN32(acc)"
        return
    # the NaN pixels are exactly the oracle's; the bounds hold on all others
    bad = np.argwhere(np.isnan(tot) != nan)
    assert len(bad) == 0, f"{tag}: NaN pixels differ from the oracle's at {bad[:4]} of {len(bad)} ({int(nan.sum())} expected)"
    keep = ~nan.reshape(-1)[P.upix]
    if direct:  # one global atomic per contribution
        J, extra = k, 0
    else:
        J, _ = case.J(int_cells, pending)
        extra = 0 if int_cells else k.astype(object)  # f64 cells: the tile sum is a sequential f64 sum
    if accum == F64A:
        assert np.array_equal(np.isnan(acc), nan), f"{tag}: NaN pixels of the accumulator differ from the oracle's"
        assert same_bits(tot, acc.astype(np.float32)), f"{tag}: map != RN32(acc)"
        err = abs(P.units(np.where(nan, 0.0, acc)) - E) * (1 << 53)
        lim = (2 * J.astype(object) + extra) * E
    else:
        got = P.units(np.where(nan, np.float32(0), tot))
        err = abs(got - E) * (1 << 53)
        lim = ((2 * J.astype(object) - 1) * (1 << 29) + extra) * E
        one = (k == 1) & keep
        assert np.all(got[one] == E[one]), f"{tag}: a pixel with a single contribution is not exact"
    bad = np.nonzero((err > lim) & keep)[0]
    if len(bad):
        w = bad[np.argmax([float(err[i]) / max(float(lim[i]), 1e-300) if lim[i] else np.inf for i in bad])]
        raise AssertionError(f"{tag}: {len(bad)} pixels outside the {ACC_IDS[accum]} bound; worst pixel {P.upix[w]}: "
                             f"k {k[w]}, J {J[w]}, |err|/E {float(err[w]) / float(E[w]) / 2.0 ** 53:.3e}")


def all_modes(S, case, sort2_too, pending=32, tag=""):
    """F32, F64 and FIXED64, each with k4_int 2 and 0; constant masses also through the run-table walk."""
    for sort2 in ((0, 1) if sort2_too and not case.hydro else (0,)):
        for accum in (F32A, F64A, FIXA):
            for k4 in (2, 0):
                tot, acc, mask = run(S, case, accum, k4, sort2, pending)
                check(case, tot, acc, mask, accum, k4, sort2, pending,
                      f"{tag} {ACC_IDS[accum]} k4_int={k4} sort2={sort2} pending={pending}")


# ---- route boundaries -------------------------------------------------------------------------------------------
NPIX, TL = 256, 6          # 4 x 4 tiles of 64 x 64 pixels
CORNER, INTERIOR = 0, 5    # tile (0, 0): clipped halo, CHECK = true; tile (1, 1): interior


@functools.lru_cache(maxsize=2)
def boundary_case(n, layout, tile, hydro):
    rng = np.random.default_rng(1000 + n % 1000 + 7 * tile + (1 if hydro else 0))
    x0 = y0 = 64 * (tile % 4)
    if layout == "pixel":
        px, py = (0, 0) if tile == CORNER else (x0 + 5, y0 + 7)
        heavy = place(n, NPIX, (px + 0.02, px + 0.98, py + 0.02, py + 0.98), rng)
    else:
        heavy = place(n, NPIX, (x0 + 0.01, x0 + 63.99, y0 + 0.01, y0 + 63.99), rng)
    in_tile = lambda xs, ys, gx, gy: ((gx >> TL) == tile % 4) & ((gy >> TL) == tile // 4)
    light = place(3000, NPIX, (0.5, NPIX - 0.5, 0.5, NPIX - 0.5), rng, reject=in_tile)
    pos = np.concatenate([light[:1500], heavy, light[1500:]])
    mass = decade_masses(len(pos), rng) if hydro else None
    return Case(NPIX, TL, pos, mass, M_CONST)


# (the integer cells' own whole-bin boundary, 32768 / 32769, is pinned in one layout)
ROUTES = [(n, "pixel", INTERIOR) for n in (32768, 32769)] + \
         [(n, layout, tile) for n in (65536, 65537, 114688, 114689, 400000) for layout in ("pixel", "spread")
          for tile in (CORNER, INTERIOR)]


@pytest.mark.parametrize("hydro", [False, True], ids=["const", "masses"])
@pytest.mark.parametrize("n,layout,tile", ROUTES, ids=[f"{n}-{l}-{'corner' if t == CORNER else 'interior'}" for n, l, t in ROUTES])
def test_route_boundaries(S, n, layout, tile, hydro):
    """Exactly n records in one (plane, tile) bin: whole, split in the plain loop, split with the wave pre-reduction;
    all in one pixel (uniform waves: one lane issues the atomics) or spread over the tile (per-lane atomics); in the
    map's corner tile (clipped halo, edge tests) and in an interior tile."""
    case = boundary_case(n, layout, tile, hydro)
    assert case.bin_count(tile) == n and len(case.xs) == n + 3000
    parts = {False: tnp.parts_of(n, False), True: tnp.parts_of(n, True)}
    want = {32768: (1, 1), 32769: (1, 3), 65536: (1, 4), 65537: (5, 5), 114688: (7, 7), 114689: (8, 8), 400000: (25, 25)}
    assert (int(parts[False]), int(parts[True])) == want[n]
    if layout == "pixel":
        hot = (0 if tile == CORNER else (64 * (tile % 4) + 5) + NPIX * (64 * (tile // 4) + 7))
        i = int(np.searchsorted(case.P.upix, hot))
        assert case.P.upix[i] == hot and case.k[i] >= n and case.k[i] > 100 * case.J(True, 32)[0][i]  # k >> J
    all_modes(S, case, sort2_too=True, tag=f"n={n} {layout}")


# ---- the noted-record list --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def noted_case(n_noted, tile, hydro):
    rng = np.random.default_rng(2000 + n_noted + tile)
    x0 = y0 = 64 * (tile % 4)
    # ordinary records in the left part of the tile, noted ones right of them; four lonely ones at the top whose
    # vanishing corner contribution is the only one its pixel receives
    def off_edges(xs, ys, gx, gy):  # (an ordinary record must not be noted by chance)
        dx, dy = xs.astype(np.float64) * NPIX - gx, ys.astype(np.float64) * NPIX - gy
        return (np.minimum(dx, 1 - dx) < 0.05) | (np.minimum(dy, 1 - dy) < 0.05)
    normal = place(6000, NPIX, (x0 + 2.05, x0 + 29.95, y0 + 2.05, y0 + 49.95), rng, reject=off_edges)
    if hydro:
        edge = place(n_noted - 4, NPIX, (x0 + 34.1, x0 + 59.9, y0 + 2.1, y0 + 49.9), rng)
        lonely = np.concatenate([place(1, NPIX, (x0 + 36.2 + 6 * i, x0 + 36.8 + 6 * i, y0 + 56.2, y0 + 56.8), rng)
                                 for i in range(4)])
        mass = np.r_[rng.uniform(1.0e-5, 1.9e-5, 6000), 10.0 ** rng.uniform(-16, -14, n_noted)].astype(np.float32)
        mass[5:6000:100] = 2000.0  # above MAX_M: count as 0 and are not noted
        mass[7:6000:100] = 0.0
        mass[0] = 1.9e-5
    else:
        # within ~2^-13 pixel right of a pixel's left edge: the weight towards the right neighbour vanishes
        def near_edge(xs, ys, gx, gy):
            d = xs.astype(np.float64) * NPIX - gx
            return (d > 0) & (d < 1.2e-4)
        cols = x0 + 34 + 2 * rng.integers(0, 12, 1)[0]
        edge = np.concatenate([place((n_noted - 4) // 4 + 1, NPIX, (c - 2e-5, c + 1.2e-4, y0 + 2.1, y0 + 49.9), rng,
                                     keep=near_edge) for c in (cols, cols + 3, cols + 6, cols + 9)])[:n_noted - 4]
        lonely = np.concatenate([place(1, NPIX, (x0 + 36 + 6 * i - 2e-5, x0 + 36 + 6 * i + 1.2e-4, y0 + 56 - 2e-5,
                                                  y0 + 56 + 1.2e-4), rng,
                                       keep=lambda xs, ys, gx, gy: near_edge(xs, ys, gx, gy) &
                                       (ys.astype(np.float64) * NPIX - gy > 0) & (ys.astype(np.float64) * NPIX - gy < 1.2e-4))
                                 for i in range(4)])
        mass = None
    pos = np.concatenate([normal, edge, lonely])
    return Case(NPIX, TL, pos, mass, 0.0156)


@pytest.mark.parametrize("hydro", [False, True], ids=["const", "masses"])
@pytest.mark.parametrize("n_noted,tile", [(511, INTERIOR), (512, INTERIOR), (513, INTERIOR), (3000, INTERIOR), (3000, CORNER)])
def test_noted_records_fill_the_list_and_overflow_inline(S, n_noted, tile, hydro):
    """n_noted records of one work item fail the branch-free loop's test (smallest product below 2^(le-25)): up to
    512 wait in the LDS list, the others are deposited inline.  A pixel that only receives a vanishing contribution
    comes out exact."""
    case = noted_case(n_noted, tile, hydro)
    assert case.bin_count(tile) == len(case.xs) <= tnp.WHOLE_RECS_INT  # one work item, whatever the cells
    assert int(case.noted.sum()) == n_noted, int(case.noted.sum())
    direct = tnp.not_quantum(case.val, case.le) & (case.pix >= 0)
    only = np.isin(case.P.upix, case.pix[direct]) & (case.k == 1)
    assert only.sum() >= 1, "no pixel with a single, vanishing contribution"
    all_modes(S, case, sort2_too=True, tag=f"noted={n_noted}")


# ---- integer-cell headroom --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def headroom_case(hydro):
    rng = np.random.default_rng(3)
    px, py = 64 + 5, 64 + 7
    pos = place(65536, NPIX, (px + 0.4, px + 0.6, py + 0.4, py + 0.6), rng)
    mass = rng.uniform(0.0150, 0.0156, len(pos)).astype(np.float32) if hydro else None
    return Case(NPIX, TL, pos, mass, 0.0156)


@pytest.mark.parametrize("hydro", [False, True], ids=["const", "masses"])
def test_integer_cells_have_headroom_for_a_whole_bin(S, hydro):
    """65536 records within 0.1 pixel of one pixel centre, masses just below 2^-6: in units of 2^(le-49) the centre
    pixel's sum exceeds 2^64, so a single workgroup's u64 cell would wrap.  (Arithmetic: 65536 * 0.5625 * 2^49 =
    1.125 * 2^64; kWholeRecsInt keeps such a bin in parts.)"""
    case = headroom_case(hydro)
    assert case.bin_count(INTERIOR) == 65536 == len(case.xs) and case.le == -6
    units = int(case.E.max()) >> (160 - 49)  # the hot pixel's exact sum in cell units
    assert units >= 1 << 64, units / 2.0 ** 64
    all_modes(S, case, sort2_too=True, tag="headroom")


# ---- several launches per pass ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def launches_case(hydro):
    rng = np.random.default_rng(4)
    n = 3 * 4 * 9000
    pos = synth.positions(0, n, BOX)
    pos[: n // 3] = place(n // 3, NPIX, (64 + 5.05, 64 + 7.95, 64 + 7.05, 64 + 8.95), rng)
    pos = pos[rng.permutation(n)]
    files = [[(9000 * (4 * f + c), 9000 * (4 * f + c + 1)) for c in range(4)] for f in range(3)]
    return Case(NPIX, TL, pos, decade_masses(n, rng) if hydro else None, M_CONST, files)


@pytest.mark.parametrize("hydro", [False, True], ids=["const", "masses"])
def test_several_launches_per_pass(S, hydro):
    """Three files of four chunks each through 12, 2 and 1 tile launches (pending 1, 8, 32): FIXED64 is the same bits
    each way (checked against the reference), F32 / F64 hold their bounds with J counted per launch."""
    case = launches_case(hydro)
    assert case.nchunks == 12
    hot = int(np.argmax(case.k))
    Js = [int(case.J(True, p)[0][hot]) for p in (1, 8, 32)]
    assert Js[0] >= 12 and Js[0] > Js[1] >= 2 and case.k[hot] > 100 * max(Js), (Js, case.k[hot])
    for pending in (1, 8, 32):
        all_modes(S, case, sort2_too=False, pending=pending, tag="launches")


# ---- NGP with per-particle masses -------------------------------------------------------------------------------
def test_ngp_with_per_particle_masses_against_exact_mass_sums(S):
    """NGP, per-particle masses (f64 cells, f32 accumulator whatever is asked for): |map - E| <= ((2J - 1) 2^-24 +
    k 2^-53) E with E the exact sum of the capped masses per pixel; the constant-mass species of the same file is bit
    for bit the oracle's."""
    rng = np.random.default_rng(5)
    n0, n1, npix = 150000, 50000, NPIX
    pos = synth.positions(0, n0 + n1, BOX)
    pos[:100000] = place(100000, npix, (64 + 5.02, 64 + 5.98, 64 + 7.02, 64 + 7.98), rng)
    m0 = decade_masses(n0, rng, top=0.05)
    f = dict(npart=[n0, n1, 0, 0, 0, 0], massarr=[0.0, M_CONST, 0, 0, 0, 0], boxsize=BOX, pos=pos, mass={0: m0})
    rc, _, ref_toti, ref_nsel = oracle.create_density_maps([f], 0, 1, npix, True, True, LD, LD2, 0, FOV, RND["sgn"],
                                                           RND["face"], RND["center"], RND["rcase"])
    assert rc == 0
    xs, ys, ms, _ = forward(pos[:n0], m0, 0.0, npix)
    gx, gy = centre_pixels(xs, ys, npix)
    inside = (gx >= 0) & (gx < npix) & (gy >= 0) & (gy < npix)
    gx, gy, ms = gx[inside], gy[inside], ms[inside]  # (NGP emits no record for an entry centred off the map)
    pix = (gx + npix * gy)[:, None]
    P = tnp.Pixels(pix, ms[:, None], npix, tnp.mass_le(ms.max()))
    E, k = P.exact(), P.count()
    tile = (gy >> TL) * 4 + (gx >> TL)
    assert int((tile == INTERIOR).sum()) > 100000  # 7 parts or more
    J, parts = tnp.addends(P, pix, ms[:, None], tile, np.zeros(len(gx), np.int64), False)
    hot = int(np.argmax(k))
    assert k[hot] >= 100000 > 100 * J[hot] and max(parts.values()) >= 7
    for accum in (F32A, F64A):
        for opt, v in (("tile_log2", TL), ("tile_h_log2", TL), ("pending", 32), ("k4_int", 2), ("sort2", 0)):
            S.set_option(opt, v)
        S.plane_begin(npix, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP, accum=accum, algo=slicer_amd.ALGO_BINNED, hydro=True)
        S.file_begin(f["npart"], f["massarr"], BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
        S.deposit_host(0, pos[:n0], m0)
        S.deposit_host(1, pos[n0:], None)
        S.file_end()
        assert (S.algo_mask() & 7) == 1 << slicer_amd.ALGO_BINNED
        tot, toti, nsel = S.plane_read(0)
        assert np.array_equal(nsel, ref_nsel)
        assert np.array_equal(toti[1].view(np.uint32), ref_toti[1].view(np.uint32))
        touched = np.zeros(npix * npix, bool)
        touched[P.upix] = True
        assert not toti[0].reshape(-1)[~touched].any()
        err = abs(P.units(toti[0]) - E) * (1 << 53)
        lim = ((2 * J.astype(object) - 1) * (1 << 29) + k.astype(object)) * E
        bad = np.nonzero(err > lim)[0]
        assert len(bad) == 0, (ACC_IDS[accum], len(bad), P.upix[bad[:4]], k[bad[:4]], J[bad[:4]])


def test_ngp_mass_sums_through_the_wave_pre_reduction(S):
    """114689 records with per-particle masses in one pixel of one interior tile of a 512^2 map: 8 parts, the fewest
    that take the heavy-bin walk, whose NGP branch sums the masses of a wave before one lane adds them.  Same bound as
    above, against the exact sum of the capped masses."""
    rng = np.random.default_rng(9)
    n, npix = 114689, 512
    px, py = 64 + 5, 64 + 7  # tile (1, 1) of 8 x 8
    pos = place(n, npix, (px + 0.02, px + 0.98, py + 0.02, py + 0.98), rng)
    m0 = decade_masses(n, rng, top=0.05)
    xs, ys, ms, _ = forward(pos, m0, 0.0, npix)
    gx, gy = centre_pixels(xs, ys, npix)
    assert len(xs) == n and np.all(gx == px) and np.all(gy == py)
    pix = (gx + npix * gy)[:, None]
    P = tnp.Pixels(pix, ms[:, None], npix, tnp.mass_le(ms.max()))
    E, k = P.exact(), P.count()
    tile = (gy >> TL) * (npix >> TL) + (gx >> TL)
    J, parts = tnp.addends(P, pix, ms[:, None], tile, np.zeros(n, np.int64), False)
    assert list(k) == [n] and list(parts.values()) == [8] and n > 100 * J[0]
    for accum in (F32A, F64A):
        for opt, v in (("tile_log2", TL), ("tile_h_log2", TL), ("pending", 32), ("k4_int", 2), ("sort2", 0)):
            S.set_option(opt, v)
        S.plane_begin(npix, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP, accum=accum, algo=slicer_amd.ALGO_BINNED, hydro=True)
        S.file_begin([n, 0, 0, 0, 0, 0], [0.0] * 6, BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
        S.deposit_host(0, pos, m0)
        S.file_end()
        assert (S.algo_mask() & 7) == 1 << slicer_amd.ALGO_BINNED
        tot, toti, nsel = S.plane_read(0)
        assert int(nsel[0]) == n and int(nsel.sum()) == n
        assert np.count_nonzero(toti[0]) == 1 and toti[0][py, px] != 0
        err = abs(P.units(toti[0]) - E) * (1 << 53)
        lim = ((2 * J.astype(object) - 1) * (1 << 29) + k.astype(object)) * E
        assert err[0] <= lim[0], (ACC_IDS[accum], float(err[0]) / float(E[0]) / 2.0 ** 53, J[0])


# ---- maps that are not a power of two wide, with masses ---------------------------------------------------------
@pytest.mark.parametrize("npix", [100, 296, 1000])
def test_ragged_edge_tiles_with_per_particle_masses(S, npix):
    """32 x 32 tiles on maps of 100, 296 and 1000 pixels (the last tile row and column are ragged), per-particle
    masses over four decades: FIXED64 bit for bit, F64 and F32 within their bounds."""
    rng = np.random.default_rng(6 + npix)
    n = 60000
    case = Case(npix, 5, synth.positions(0, n, BOX), decade_masses(n, rng), M_CONST)
    ntx = (npix + 31) >> 5
    assert npix % 32 and case.bin_count(ntx * ntx - 1) > 0 and len(case.xs) > n // 10
    assert ((case.gx < 0) | (case.gx >= npix) | (case.gy < 0) | (case.gy >= npix)).any()  # records centred off the map
    all_modes(S, case, sort2_too=False, tag=f"npix={npix}")
