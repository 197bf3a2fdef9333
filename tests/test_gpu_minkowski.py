"""slicer_minkowski_* on the device against the restatement tests/minkowski_np.py.  Every count is
an integer, so everything here is exact: np.array_equal on int64, nowhere a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import minkowski_np as MK
import moments_np as M
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
# The cell grid is n + 1 wide: tile seams fall between n = 15 / 16 (rows) and 63 / 64 (columns); maps that are all border
# (1, 2); both load paths (4 | n or not); more tiles than workgroups (4096: 16705 tiles).  The grid is at most 8
# workgroups a CU (5 at T = 1025, whose LDS is 31172 B), 2048 and 1280 on 256 CUs, so the tile loop takes a second round
# from 2049 (1281) tiles on: 4096 runs it eight to fourteen times on the float4 path; 1425 (1426 cells: 90 x 23 = 2070
# tiles, the smallest odd n past 2048) runs it twice on the scalar path with a short last tile row and column
SMALL = [1, 2, 3, 4, 5, 15, 16, 17, 18, 33, 63, 64, 65, 66, 67, 68, 100, 129]
KINDS = ("white", "lognormal", "integers")
COUNTS = (1, 2, 8, 65, 1025)


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=4)
def make_map(n, kind, seed=0):
    rng = np.random.default_rng(7919 * n + seed)
    if kind == "integers":  # many ties, and thresholds that equal pixel values
        x = rng.integers(-3, 4, (n, n))
    else:
        g = rng.standard_normal((n, n), np.float32)
        x = g if kind == "white" else np.exp(g) - np.float32(np.exp(0.5))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def make_thresholds(kind, T, spacing):
    """Thresholds that leave some pixels below the first and above the last; on the integer maps several are pixel values."""
    lo, hi = {"white": (-2.5, 3.0), "lognormal": (-1.25, 6.0), "integers": (-2.0, 2.0)}[kind]
    if T == 1:
        return np.array([0.5 * (lo + hi)])
    if spacing == "uniform":
        t = lo + np.arange(T, dtype=np.float64) * ((hi - lo) / (T - 1))
    else:
        t = lo + (hi - lo) * (np.geomspace(1.0, 100.0, T) - 1.0) / 99.0  # log-spaced
    t[0], t[-1] = lo, hi
    assert np.all(np.diff(t) > 0)
    return t


def run(s, x, thresholds, off_grid=False):
    """read() of one run on a fresh handle."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Minkowski(s, n, thresholds) as m:
            m.run(d + 4 if off_grid else d)
            return m.read()
    finally:
        s.free(d)


def check(s, x, thresholds, off_grid=False):
    got = run(s, x, thresholds, off_grid)
    ref = MK.counts(x, thresholds)
    for k in MK.KEYS:
        assert np.array_equal(got[k], ref[k]), (x.shape[0], len(thresholds), k, got[k], ref[k])
    assert all(got[k].dtype == np.int64 and got[k].shape == (len(thresholds),) for k in MK.KEYS[:-1])
    assert np.array_equal(got["thresholds"], thresholds) and got["npix"] == x.shape[0]
    assert np.array_equal(got["euler"], got["vertices"] - got["edges"] + got["faces"])
    return got


@pytest.mark.parametrize("n", SMALL)
def test_counts_are_the_restatement(slicer, n):
    for kind in KINDS:
        x = make_map(n, kind)
        for T in COUNTS:
            for spacing in ("uniform", "log"):
                check(slicer, x, make_thresholds(kind, T, spacing))


@pytest.mark.parametrize("n,kind,T,spacing", [
    (1000, "white", 8, "log"), (1000, "lognormal", 1025, "uniform"), (1000, "integers", 65, "uniform"),
    (1023, "white", 1025, "log"), (1023, "lognormal", 1, "uniform"), (1023, "integers", 8, "uniform"),
    (1024, "white", 65, "uniform"), (1024, "lognormal", 2, "log"), (1024, "integers", 1025, "log"),
    (1425, "white", 8, "log"), (1425, "lognormal", 1025, "uniform"),
    (4096, "white", 1025, "uniform"), (4096, "lognormal", 65, "log"), (4096, "integers", 1, "uniform"),
])
def test_counts_of_large_maps_are_the_restatement(slicer, n, kind, T, spacing):
    got = check(slicer, make_map(n, kind), make_thresholds(kind, T, spacing))
    assert 0 < got["faces"][-1] <= got["faces"][0] < n * n and got["boundary"][0] > 0


@pytest.mark.parametrize("n", [130, 257, 1024])
def test_plateaus_take_the_shortcut_of_equal_ranks_and_every_number_of_counter_copies(slicer, n):
    # blocks of 8 x 8 equal pixels, offset by 3 so that they straddle the tile seams: most threads see ten equal ranks.
    # T = 3, 65, 129, 257, 1025 keep 32, 8, 4, 2 and 1 copies of the counters
    rng = np.random.default_rng(n)
    coarse = rng.integers(-3, 4, (n // 8 + 2, n // 8 + 2)).astype(np.float32)
    x = np.kron(coarse, np.ones((8, 8), np.float32))[3:3 + n, 3:3 + n].copy()
    assert x.shape == (n, n)
    for T in (3, 65, 129, 257, 1025):
        got = check(slicer, x, make_thresholds("integers", T, "uniform"))
        assert 0 < got["faces"][-1] < got["faces"][0] < n * n
    # one plateau: the whole map at one rank, every lane on the same counters
    flat = np.full((n, n), 0.25, np.float32)
    for T in (1, 65, 1025):
        t = make_thresholds("integers", T, "uniform")
        got = check(slicer, flat, t)
        k = int(np.searchsorted(t, 0.25, "right"))
        want = {"faces": n * n, "edges": 2 * n * (n + 1), "vertices": (n + 1) ** 2, "boundary": 0, "border": 4 * n, "euler": 1}
        for name, v in want.items():
            assert np.all(got[name][:k] == v) and not got[name][k:].any() and k >= 1


# n = 130: the cells are 131 x 131, the tile seams lie between cell rows 15 / 16, 31 / 32, ..., 127 / 128 and cell columns
# 63 / 64 and 127 / 128; a pixel (i, j) is cell (i, j)'s face, and its bottom and right sides belong to cells (i+1, j), (i, j+1)
N = 130
INTERIOR, CORNER, SIDE = (1, 4, 4, 4, 0, 1), (1, 4, 4, 2, 2, 1), (1, 4, 4, 3, 1, 1)
SHAPES = {
    "corners": ([(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)], [CORNER] * 4),
    # both sides of the seams: cell columns 63 / 64 and 127 / 128 along the top and the bottom, cell rows 15 / 16 and
    # 127 / 128 along the left and the right
    "sides": ([(0, 5), (0, 63), (0, 127), (N - 1, 90), (N - 1, 64), (N - 1, 128), (9, 0), (15, 0), (128, 0), (70, N - 1),
               (16, N - 1), (127, N - 1)], [SIDE] * 12),
    "seams": ([(15, 40), (16, 44), (40, 63), (44, 64), (15, 63), (32, 64), (15, 127), (32, 128), (100, 127), (104, 128),
               (31, 5), (32, 9), (127, 63), (128, 70), (14, 60), (64, 126), (127, 127), (1, 1), (128, 124)], [INTERIOR] * 19),
}


def by_hand(shapes):
    """The six counts (faces, edges, vertices, boundary, border, euler) of shapes that do not touch one another, per
    threshold j: shape k (height k + 1) is in the sets 0 ... k of the thresholds 0.5, 1.5, ..."""
    H = len(shapes)
    out = np.zeros((6, H), np.int64)
    for k, six in enumerate(shapes):
        out[:, :k + 1] += np.array(six, np.int64)[:, None]
    return out


def six_of(r):
    return np.stack([r[k] for k in ("faces", "edges", "vertices", "boundary", "border", "euler")])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_planted_single_pixels_are_counted_where_they_stand(slicer, name):
    at, shapes = SHAPES[name]
    H = len(at)
    t = np.arange(H, dtype=np.float64) + 0.5  # pixel k, of height k + 1, is in the sets 0 ... k
    x = np.zeros((N, N), np.float32)
    for k, a in enumerate(at):
        x[a] = 1.0 + k
    got = run(slicer, x, t)
    assert np.array_equal(six_of(got), by_hand(shapes)), (name, six_of(got))
    assert MK.same(got, MK.counts(x, t))
    # the sign flipped and the thresholds negated: the sets x >= -t_j are the complements' closures, so only the
    # restatement is the reference there, and the top threshold gives the whole map but the H planted pixels' absence
    flipped = run(slicer, -x, -t[::-1])
    assert MK.same(flipped, MK.counts(-x, -t[::-1]))
    assert flipped["faces"][0] == N * N - 1 and flipped["faces"][-1] == N * N - H


def test_planted_pairs_and_rings_across_the_seams(slicer):
    # diagonal pairs: two faces, eight edges, seven vertices (the shared corner once), one component
    pairs = [((15, 20), (16, 21)), ((40, 63), (41, 64)), ((15, 127), (16, 128)), ((31, 64), (32, 63)), ((70, 70), (71, 71))]
    pair = (2, 8, 7, 8, 0, 1)
    # rings of eight pixels around an empty centre: sixteen vertices, twenty-four edges, one hole
    rings = [(16, 64), (32, 127), (48, 63), (127, 127), (80, 20)]  # their centres
    ring = (8, 24, 16, 16, 0, 0)
    shapes, x = [], np.zeros((N, N), np.float32)
    for a, b in pairs:
        shapes.append(pair)
        x[a] = x[b] = len(shapes)
    for ci, cj in rings:
        shapes.append(ring)
        x[ci - 1:ci + 2, cj - 1:cj + 2] = len(shapes)
        x[ci, cj] = 0.0
    t = np.arange(len(shapes), dtype=np.float64) + 0.5
    got = run(slicer, x, t)
    assert np.array_equal(six_of(got), by_hand(shapes)), six_of(got)
    assert MK.same(got, MK.counts(x, t))
    flipped = run(slicer, -x, -t[::-1])
    assert MK.same(flipped, MK.counts(-x, -t[::-1]))


def test_a_pixel_on_a_threshold_is_in_its_set(slicer):
    f32 = np.float32
    t = np.array([0.25, 0.5, 1.0, 2.0])  # all of them f32 values
    up = [np.nextafter(f32(e), f32(np.inf)) for e in t]
    down = [np.nextafter(f32(e), f32(-np.inf)) for e in t]
    x = np.full((8, 8), 0.75, f32)  # rank 2
    x[0, :4], x[2, :4], x[4, :4] = t, up, down
    got = check(slicer, x, t)
    # ranks: on the thresholds 1, 2, 3, 4; just above the same; just below 0, 1, 2, 3; the 52 others 2
    assert list(got["faces"]) == [63, 3 + 3 + 2 + 52, 2 + 2 + 1, 1 + 1]


def test_the_thresholds_are_compared_in_f64(slicer):
    f32 = np.float32
    x = f32(0.1)
    above_x, below_x = np.float64(x) * (1 + 2.0 ** -30), np.float64(x) * (1 - 2.0 ** -30)
    assert f32(above_x) == x == f32(below_x) and below_x < np.float64(x) < above_x  # rounded to f32 both are x
    m = np.full((5, 5), x, f32)
    for t, faces in ((above_x, 0), (below_x, 25)):
        got = check(slicer, m, np.array([t]))
        assert got["faces"][0] == faces and got["euler"][0] == (1 if faces else 0)
    # the same in the middle of the binary search's deeper levels
    for T in (8, 1025):
        base = np.linspace(0.0, 1.0, T)
        k = int(np.searchsorted(base, np.float64(x)))
        assert 0 < k < T - 1
        for t, in_set_k in ((above_x, 0), (below_x, 25)):
            thr = base.copy()
            thr[k] = t
            got = check(slicer, m, thr)
            assert got["faces"][k] == in_set_k and got["faces"][k - 1] == 25 and got["faces"][k + 1] == 0


def test_nan_and_infinite_pixels(slicer):
    n = 33
    x = make_map(n, "white").copy()
    nans, pinf, ninf = [(5, 5), (16, 16), (0, 3), (32, 32), (15, 31), (20, 0)], [(8, 20), (20, 8), (0, 0)], [(25, 25), (31, 1), (32, 9)]
    for at in nans:
        x[at] = np.nan
    for at in pinf:
        x[at] = np.inf
    for at in ninf:
        x[at] = -np.inf
    t = np.linspace(-1.0, 1.0, 8)
    got = check(slicer, x, t)
    assert got["nan"] == len(nans)
    below = int((x.astype(np.float64) < t[0]).sum())  # (NaN: False)
    assert got["faces"][0] + below + got["nan"] == n * n
    assert got["faces"][-1] >= len(pinf)  # +inf is in every set
    # a map of NaN and -inf alone is in no set
    y = np.full((n, n), np.nan, np.float32)
    y[::2] = -np.inf
    empty = check(slicer, y, t)
    assert not any(empty[k].any() for k in MK.KEYS[:-1]) and empty["nan"] == int(np.isnan(y).sum())


@pytest.mark.parametrize("n", [64, 1024])
def test_an_input_off_the_16_byte_grid_gives_the_same_counts(slicer, n):
    x = make_map(n, "lognormal")
    t = make_thresholds("lognormal", 65, "log")
    on, off = run(slicer, x, t), run(slicer, x, t, off_grid=True)
    assert MK.same(on, off) and MK.same(on, MK.counts(x, t))


def test_runs_repeat_and_carry_nothing_over(slicer):
    n = 257
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    t = make_thresholds("white", 65, "uniform")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        with slicer_amd.Minkowski(slicer, n, t) as m:
            m.run(dx)
            first = m.read()
            m.run(dx)
            assert MK.same(first, m.read())
            m.run(dy)  # a second, different map on the same handle
            second = m.read()
        assert MK.same(first, MK.counts(x, t)) and MK.same(second, run(slicer, y, t))
        assert not MK.same(first, second)
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def test_run_npix_on_a_smaller_map_is_a_handle_of_that_size(slicer):
    t = make_thresholds("white", 65, "log")
    maps = {m: make_map(m, "white") for m in (200, 67, 64, 3, 1)}
    ptrs = {m: slicer.to_device(x) for m, x in maps.items()}
    try:
        with slicer_amd.Minkowski(slicer, 200, t) as mk:
            for m in (200, 67, 64, 3, 1, 200):
                mk.run(ptrs[m], m)
                got = mk.read()
                assert MK.same(got, run(slicer, maps[m], t)) and got["npix"] == m
    finally:
        for d in ptrs.values():
            slicer.free(d)


@pytest.mark.parametrize("n", [66, 1000])
def test_run_level_over_a_moments_pyramid(slicer, n):
    x = make_map(n, "lognormal")
    levels = int(np.log2(n))
    t = make_thresholds("lognormal", 65, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, levels) as m, slicer_amd.Minkowski(slicer, n, t) as mk:
            m.run(d)
            mk.run(d)
            assert MK.same(mk.read(), MK.counts(x, t))
            pyr = M.pyramid(x, levels, "mean")
            for level in range(1, levels + 1):
                mk.run_level(m, level)
                got = mk.read()
                y = m.read_map(level)
                assert y.tobytes() == pyr[level].tobytes()
                assert MK.same(got, MK.counts(y, t)) and got["npix"] == n >> level
    finally:
        slicer.free(d)


def test_run_kappa_is_run_on_the_kappa_map(slicer):
    n = 48
    x = make_map(n, "lognormal")
    t = make_thresholds("lognormal", 8, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Minkowski(slicer, n, t) as mk:
            kappa.add_device([d], [[1.0]])
            mk.run_kappa(kappa, 0)
            a = mk.read()
            mk.run(kappa.device_map(0))
            assert MK.same(a, mk.read()) and MK.same(a, MK.counts(kappa.read(0), t))
            assert a["faces"][0] > a["faces"][-1] > 0
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.ones(n * n, np.float32))
    t = np.array([0.0, 1.0, 2.0])
    mh = C.c_void_p()
    assert L.slicer_minkowski_create(slicer._h, n, 3, t.ctypes.data, C.byref(mh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.zeros(3, np.int64)
        assert L.slicer_minkowski_read(mh, buf.ctypes.data, None, None, None, None, None) == ERR_STATE
        assert err() == "slicer_minkowski_read before any slicer_minkowski_run"
        assert L.slicer_minkowski_run(mh, None) == ERR_ARG
        assert err() == "slicer_minkowski_run: null argument"
        assert L.slicer_minkowski_run_npix(mh, None, 4) == ERR_ARG
        assert err() == "slicer_minkowski_run_npix: null argument"
        for bad in (0, -1, 17):
            assert L.slicer_minkowski_run_npix(mh, d, bad) == ERR_ARG
            assert err() == f"slicer_minkowski_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_minkowski_read(mh, buf.ctypes.data, None, None, None, None, None) == ERR_STATE
        assert L.slicer_minkowski_run(mh, d) == 0
        assert L.slicer_minkowski_read(mh, buf.ctypes.data, None, None, None, None, None) == 0
        assert list(buf) == [n * n, n * n, 0]
        border, nan = np.zeros(3, np.int64), C.c_int64(-1)
        assert L.slicer_minkowski_read(mh, None, None, None, None, border.ctypes.data, C.byref(nan)) == 0
        assert list(border) == [4 * n, 4 * n, 0] and nan.value == 0
        out = C.c_void_p(1)
        assert L.slicer_minkowski_create(slicer._h, n, 3, t[::-1].copy().ctypes.data, C.byref(out)) == ERR_ARG
        assert err() == "slicer_minkowski_create: thresholds must be strictly ascending"
        assert not out.value
        assert L.slicer_minkowski_create(slicer._h, n, 3, t.ctypes.data, None) == ERR_ARG
        assert err() == "slicer_minkowski_create: null argument"
    finally:
        L.slicer_minkowski_destroy(mh)
        slicer.free(d)
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Minkowski(slicer, n, [0.0, np.nan])
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Minkowski(slicer, n, [])


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n, "white"))
    try:
        with slicer_amd.Minkowski(slicer, n, make_thresholds("white", 8, "uniform")) as m:
            slicer.profile_reset()
            slicer.profile_enable(True)
            m.run(d)
            m.run(d, 32)
            m.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["minkowski"][0] == 2 and prof["minkowski_finish"][0] == 2
    finally:
        slicer.free(d)
