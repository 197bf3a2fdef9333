"""slicer_starlet_* on the device against the restatement tests/starlet_np.py.  Everything is
compared as values (==) with equal NaN positions: nowhere a tolerance."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import moments_np as M
import slicer_amd
import starlet_np as W
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
# n below the reach of every level; both sides of the tile seams of level_cfg: a tile is 128 columns (one span up to
# d = 16, eight runs of 16 at stride d above) by two segments of at most 8 rows at stride d, so at step d the seams are
# at columns 128 k (d <= 16) and 8 d k (d = 32: 256), and at rows 16 d k: 16, 32, 64, 96, 128, 256 for d = 1 ... 16; maps
# with fewer than 16 rows per residue (n < 16 d) take shorter segments, n < d leaves residues empty.
# The dilated regime (d >= 32): a residue has ceil(n / d) rows and columns, a tile takes 16 and 8 of them, so a second row
# block needs n > 16 d = 512 and the sizes here stay at one row block at d = 32.  (1024, 8) of the large maps has two, all
# of them full.  DILATED has the ragged ones: 530 at d = 32 (17 a residue: a second row block of one row in residues
# 0 ... 17 and of none in 18 ... 31, three column blocks, the last of one column), 1031 at d = 32 (33: three row blocks,
# five column blocks) and at d = 64 (17, the extra row and column in residues 0 ... 6)
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 127, 128, 129, 130, 255, 256, 257, 260]
SCALES = (1, 3, 6)
DILATED = [(530, 6), (1031, 7)]


def level_counts(n, j):
    """level_cfg of slicer_amd/csrc/slicer_starlet.hip at level j (d = 2^j) of an n x n map: the rows of a residue at
    most, the rows of a segment, and the tiles as row blocks x column residue runs x column blocks a row residue."""
    d, run_log2 = 1 << j, min(j, 4)
    tc, run = 128 >> run_log2, 1 << run_log2
    per_residue = (n + d - 1) // d
    seg = max(1, min(8, (per_residue + 1) // 2))
    return {"per_residue": per_residue, "seg": seg, "kblocks_r": (per_residue + 2 * seg - 1) // (2 * seg),
            "resblocks_c": (min(d, n) + run - 1) // run, "kblocks_c": (per_residue + tc - 1) // tc}


# what the comment above claims (no device needed)
assert all(level_counts(n, 5)["kblocks_r"] == 1 for n in SIZES) and level_counts(512, 5)["kblocks_r"] == 1
assert level_counts(1024, 5) == {"per_residue": 32, "seg": 8, "kblocks_r": 2, "resblocks_c": 2, "kblocks_c": 4}
assert level_counts(530, 5) == {"per_residue": 17, "seg": 8, "kblocks_r": 2, "resblocks_c": 2, "kblocks_c": 3}
assert level_counts(1031, 5) == {"per_residue": 33, "seg": 8, "kblocks_r": 3, "resblocks_c": 2, "kblocks_c": 5}
assert level_counts(1031, 6) == {"per_residue": 17, "seg": 8, "kblocks_r": 2, "resblocks_c": 4, "kblocks_c": 3}
assert 530 % 32 == 18 and 1031 % 32 == 7 and 1031 % 64 == 7  # the residues below these hold the extra row and column


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=4)
def make_map(n, kind="lognormal", seed=0):
    rng = np.random.default_rng(7907 * n + seed)
    g = rng.standard_normal((n, n), np.float32)
    x = (g if kind == "white" else np.exp(g) - np.float32(math.exp(0.5))).astype(np.float32)
    x.setflags(write=False)
    return x


def same(got, ref):
    """Equal values and equal NaN positions (the sign of a zero and NaN payloads carry no contract)."""
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and bool(
        np.all((got == ref) | (np.isnan(got) & np.isnan(ref))))


def run(s, x, scales, off_grid=False):
    """read_all() of one run on a fresh handle."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Starlet(s, n, scales) as st:
            st.run(d + 4 if off_grid else d)
            return st.read_all()
    finally:
        s.free(d)


def check(s, x, scales, off_grid=False, ref=None):
    got = run(s, x, scales, off_grid)
    ref = W.starlet(x, scales) if ref is None else ref
    assert len(got) == len(ref) == scales + 1
    for j in range(scales + 1):
        if not same(got[j], ref[j]):
            bad = ~((got[j] == ref[j]) | (np.isnan(got[j]) & np.isnan(ref[j])))
            raise AssertionError((x.shape[0], scales, off_grid, j, int(bad.sum()), np.argwhere(bad)[:4].tolist()))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_maps_are_the_restatement(slicer, n):
    for kind in ("white", "lognormal"):
        x = make_map(n, kind)
        for scales in SCALES:
            ref = W.starlet(x, scales)
            for off_grid in (False, True):
                check(slicer, x, scales, off_grid, ref)


@pytest.mark.parametrize("n", [5, 33, 257])
def test_twelve_scales(slicer, n):
    for kind in ("white", "lognormal"):
        x = make_map(n, kind)
        ref = W.starlet(x, 12)
        for off_grid in (False, True):
            check(slicer, x, 12, off_grid, ref)


@pytest.mark.parametrize("n,scales", [(1024, 8), (1000, 4)])
def test_large_maps_are_the_restatement(slicer, n, scales):
    x = make_map(n)
    got = check(slicer, x, scales)
    assert all(np.isfinite(g).all() and float(np.abs(g).max()) > 0 for g in got)
    # the scales sum back to the map within the J + 1 roundings to f32
    total = sum(g.astype(np.float64) for g in got)
    bound = 2.0 ** -24 * sum(np.abs(g).astype(np.float64) for g in got) * (1 + 2.0 ** -20)
    assert (np.abs(total - x.astype(np.float64)) <= bound).all()


@pytest.mark.parametrize("n,scales", DILATED)
def test_dilated_tiles_past_one_block_on_ragged_maps(slicer, n, scales):
    """At d >= 32 blockIdx.x decodes into (column block, column residue run, row block, row residue) with more than one
    row block and more than one column block, and n mod d != 0 leaves the last of each ragged: one row (column) in the
    low residues, none in the others, where `row >= n` and `col >= n` cut the tile short."""
    for j in range(5, scales):
        c = level_counts(n, j)
        assert c["kblocks_r"] >= 2 and c["kblocks_c"] >= 2 and c["resblocks_c"] >= 2 and n % (1 << j) != 0, (j, c)
        assert (c["per_residue"] - 1) % (2 * c["seg"]) == 0  # the last row block holds one row
    for kind in ("white", "lognormal"):
        x = make_map(n, kind)
        ref = W.starlet(x, scales)
        for off_grid in (False, True):
            check(slicer, x, scales, off_grid, ref)


@pytest.mark.parametrize("n", [5, 130])
def test_a_constant_map_is_its_own_coarse_map(slicer, n):
    for value in (3.25, 0.1, -1e30):
        x = np.full((n, n), value, np.float32)
        got = run(slicer, x, 8)
        assert got[0].tobytes() == x.tobytes(), (n, value)
        assert all(not w.any() for w in got[1:])


def test_run_npix_on_a_smaller_map_is_a_handle_of_that_size(slicer):
    maps = {m: make_map(m) for m in (200, 129, 64, 3, 1)}
    ptrs = {m: slicer.to_device(x) for m, x in maps.items()}
    try:
        with slicer_amd.Starlet(slicer, 200, 5) as st:
            for m in (200, 129, 64, 3, 1, 200, 3, 129):  # smaller after larger and back
                st.run(ptrs[m], m)
                got, fresh = st.read_all(), run(slicer, maps[m], 5)
                for j in range(6):
                    assert got[j].shape == (m, m) and got[j].tobytes() == fresh[j].tobytes(), (m, j)
    finally:
        for d in ptrs.values():
            slicer.free(d)


def test_run_level_over_a_moments_pyramid(slicer):
    n, levels = 66, 3
    x = make_map(n)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, levels) as m, slicer_amd.Starlet(slicer, n, 3) as st:
            m.run(d)
            pyr = M.pyramid(x, levels, "mean")
            for level in range(1, levels + 1):
                st.run_level(m, level)
                ref = W.starlet(pyr[level], 3)
                got = st.read_all()
                assert all(same(got[j], ref[j]) for j in range(4)), level
    finally:
        slicer.free(d)


def test_runs_repeat_and_carry_nothing_over(slicer):
    n, scales = 257, 6
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        with slicer_amd.Starlet(slicer, n, scales) as st:
            st.run(dx)
            first = st.read_all()
            st.run(dx)
            again = st.read_all()
            st.run(dy)  # a second, different map on the same handle
            second = st.read_all()
        fresh = run(slicer, y, scales)
        for j in range(scales + 1):
            assert again[j].tobytes() == first[j].tobytes() and second[j].tobytes() == fresh[j].tobytes()
            assert first[j].tobytes() != second[j].tobytes()
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def reach_of_one_pixel(slicer, n, scales, pixels, value):
    clean = make_map(n)
    before = run(slicer, clean, scales)
    for at in pixels:
        x = clean.copy()
        x[at] = value
        got = check(slicer, x, scales)
        reach = W.reach(x, scales)
        for j in range(scales + 1):
            assert np.array_equal(~np.isfinite(got[j]), reach[j]), (at, j)
            assert got[j][~reach[j]].tobytes() == before[j][~reach[j]].tobytes()  # every other output keeps its bits
            if value != value:
                assert np.isnan(got[j][reach[j]]).all()


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_pixel_reaches_exactly_its_support(slicer, value):
    # corners, both sides of a tile seam, the middle
    reach_of_one_pixel(slicer, 150, 5, ((0, 0), (31, 128), (32, 127), (149, 64), (75, 75)), value)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_pixel_reaches_exactly_its_support_in_ragged_dilated_tiles(slicer, value):
    # n = 530 at d = 32 (DILATED): row 528 = 16 + 16 d is the one row of residue 16's second row block, column 529 =
    # 17 + 16 d the one column of residue 17's third column block, (529, 529) both at once, in the corner
    reach_of_one_pixel(slicer, 530, 6, ((528, 300), (17, 529), (529, 529)), value)


def test_run_kappa_and_a_second_handle_on_a_scale(slicer):
    n = 48
    x = make_map(n)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Starlet(slicer, n, 3) as a, \
                slicer_amd.Starlet(slicer, n, 2) as b:
            kappa.add_device([d], [[1.0]])
            a.run_kappa(kappa, 0)
            first = a.read_all()
            ref = W.starlet(kappa.read(0), 3)
            assert all(same(first[j], ref[j]) for j in range(4))
            b.run(a.device_map(2), n)  # a scale, where it is
            ref_b = W.starlet(first[2], 2)
            assert all(same(got, r) for got, r in zip(b.read_all(), ref_b))
            # a handle does not take its own outputs as its input
            err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
            for scale in range(4):
                assert L.slicer_starlet_run(a._sh, a.device_map(scale)) == ERR_ARG and "overlaps" in err()
            assert L.slicer_starlet_run_npix(a._sh, a.device_map(3) + 4 * n * n - 4, 1) == ERR_ARG
            assert L.slicer_starlet_run_npix(a._sh, a.device_map(0) - 4, 2) == ERR_ARG
            assert all(a.read(j).tobytes() == first[j].tobytes() for j in range(4))
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    sh = C.c_void_p()
    assert L.slicer_starlet_create(slicer._h, n, 2, C.byref(sh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.ones((n, n), np.float32)
        p = C.c_void_p()
        for scale in (0, 1, 2):
            assert L.slicer_starlet_read(sh, scale, buf.ctypes.data) == ERR_STATE
            assert err() == "slicer_starlet_read before any slicer_starlet_run"
            assert L.slicer_starlet_device_map(sh, scale, C.byref(p)) == ERR_STATE
            assert err() == "slicer_starlet_device_map before any slicer_starlet_run"
        assert L.slicer_starlet_run(sh, None) == ERR_ARG and err() == "slicer_starlet_run: null argument"
        assert L.slicer_starlet_run_npix(sh, None, 4) == ERR_ARG and err() == "slicer_starlet_run_npix: null argument"
        for bad in (0, -1, 17):
            assert L.slicer_starlet_run_npix(sh, d, bad) == ERR_ARG
            assert err() == f"slicer_starlet_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_starlet_read(sh, 0, buf.ctypes.data) == ERR_STATE
        assert L.slicer_starlet_run(sh, d) == 0
        assert L.slicer_starlet_read(sh, 0, None) == ERR_ARG and L.slicer_starlet_device_map(sh, 0, None) == ERR_ARG
        for bad in (-1, 3):
            assert L.slicer_starlet_read(sh, bad, buf.ctypes.data) == ERR_ARG
            assert err() == f"slicer_starlet_read: scale = {bad} outside 0..2"
            assert L.slicer_starlet_device_map(sh, bad, C.byref(p)) == ERR_ARG
            assert err() == f"slicer_starlet_device_map: scale = {bad} outside 0..2"
        for scale in (0, 1, 2):
            buf[:] = 1
            assert L.slicer_starlet_read(sh, scale, buf.ctypes.data) == 0 and not buf.any()
            assert L.slicer_starlet_device_map(sh, scale, C.byref(p)) == 0 and p.value
        out = C.c_void_p(1)
        assert L.slicer_starlet_create(slicer._h, n, 13, C.byref(out)) == ERR_ARG and not out.value
        assert err() == "slicer_starlet_create: scales = 13 outside 1..12"
        assert L.slicer_starlet_create(slicer._h, n, 2, None) == ERR_ARG
        assert err() == "slicer_starlet_create: null argument"
    finally:
        L.slicer_starlet_destroy(sh)
        slicer.free(d)
    for bad in (0, 13):
        with pytest.raises(slicer_amd.SlicerError):
            slicer_amd.Starlet(slicer, n, bad)


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n))
    try:
        with slicer_amd.Starlet(slicer, n, 4) as a, slicer_amd.Starlet(slicer, n, 1) as b:
            slicer.profile_reset()
            slicer.profile_enable(True)
            a.run(d)
            a.run(d, 32)
            b.run(d)
            a.read(0)
            b.read(0)
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["starlet_first"][0] == 3 and prof["starlet_level"][0] == 4 and prof["starlet_last"][0] == 2
    finally:
        slicer.free(d)
