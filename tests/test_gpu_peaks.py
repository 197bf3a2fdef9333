"""slicer_peaks_* on the device against the restatement tests/peaks_np.py.  Every count is an
integer, so everything here is exact: np.array_equal on int64, nowhere a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import moments_np as M
import peaks_np as P
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
KEYS = ("pdf", "peaks", "minima", "below", "above", "nan")
# no interior (1, 2), one interior pixel (3), tile seams at rows 16 / 32 and columns 64 / 128, both load paths
# (4 | n or not), more tiles than workgroups (4096: 16384 tiles).  The grid is at most 8 workgroups a CU (6 at
# B = 1024, whose LDS is 25700 B), 2048 and 1536 on 256 CUs, so the tile loop takes a second round from 2049 (1537) tiles
# on: 4096 runs it eight to eleven times, on the float4 path with every tile full; 1425 (90 x 23 = 2070 tiles, the
# smallest n past 2048) runs it twice on the scalar path with a short last tile row and column
SMALL = [1, 2, 3, 4, 5, 15, 16, 17, 18, 33, 63, 64, 65, 66, 67, 68, 100, 129]
KINDS = ("white", "lognormal", "integers")
BINS = (1, 7, 64, 1024)


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=4)
def make_map(n, kind, seed=0):
    rng = np.random.default_rng(7919 * n + seed)
    if kind == "integers":  # many ties
        x = rng.integers(-3, 4, (n, n))
    else:
        g = rng.standard_normal((n, n), np.float32)
        x = g if kind == "white" else np.exp(g) - np.float32(np.exp(0.5))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4)
def masks(n, kind, seed=0):
    return P.extrema(make_map(n, kind, seed))


def make_edges(kind, B, spacing):
    """Edges that leave some pixels below and above; on the integer maps several edges are pixel values."""
    lo, hi = {"white": (-2.5, 3.0), "lognormal": (-1.25, 6.0), "integers": (-2.0, 2.0)}[kind]
    if spacing == "uniform":
        return P.uniform_edges(lo, hi, B)
    e = lo + (hi - lo) * (np.geomspace(1.0, 100.0, B + 1) - 1.0) / 99.0  # log-spaced
    e[0], e[B] = lo, hi
    assert np.all(np.diff(e) > 0)
    return e


def same(got, ref):
    return all(np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)) for k in KEYS)


def total(r):
    return int(r["pdf"].sum() + r["below"][0] + r["above"][0] + r["nan"])


def run(s, x, edges, off_grid=False):
    """read() of one run on a fresh handle."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Peaks(s, n, edges) as p:
            p.run(d + 4 if off_grid else d)
            return p.read()
    finally:
        s.free(d)


def check(s, x, edges, ref_masks=None, off_grid=False):
    got = run(s, x, edges, off_grid)
    ref = P.counts(x, edges, ref_masks)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), (x.shape[0], len(edges) - 1, k, got[k], ref[k])
    assert got["pdf"].dtype == got["peaks"].dtype == got["minima"].dtype == got["below"].dtype == np.int64
    assert np.array_equal(got["edges"], edges)
    assert total(got) == x.size
    return got


@pytest.mark.parametrize("n", SMALL)
def test_counts_are_the_restatement(slicer, n):
    for kind in KINDS:
        x = make_map(n, kind)
        for B in BINS:
            for spacing in ("uniform", "log"):
                check(slicer, x, make_edges(kind, B, spacing), masks(n, kind))


@pytest.mark.parametrize("n,kind,B,spacing", [
    (1000, "white", 7, "log"), (1000, "lognormal", 1024, "uniform"), (1000, "integers", 64, "uniform"),
    (1023, "white", 1024, "log"), (1023, "lognormal", 1, "uniform"), (1023, "integers", 7, "uniform"),
    (1024, "white", 64, "uniform"), (1024, "lognormal", 7, "log"), (1024, "integers", 1024, "log"),
    (1425, "white", 7, "log"), (1425, "lognormal", 1024, "uniform"),
    (4096, "white", 1024, "uniform"), (4096, "lognormal", 64, "log"), (4096, "integers", 1, "uniform"),
])
def test_counts_of_large_maps_are_the_restatement(slicer, n, kind, B, spacing):
    got = check(slicer, make_map(n, kind), make_edges(kind, B, spacing), masks(n, kind))
    assert got["below"][0] > 0 and got["above"][0] > 0
    if kind != "integers":  # a ninth of the interior each
        for k, name in ((1, "peaks"), (2, "minima")):
            assert got[name].sum() + got["below"][k] + got["above"][k] > (n - 2) ** 2 // 10


def spikes(n, at, sign=1.0):
    x = np.zeros((n, n), np.float32)
    for k, (i, j) in enumerate(at):
        x[i, j] = sign * (1.0 + k)  # spike k has height k + 1: bin k of the edges 0.5, 1.5, ...
    return x


def test_planted_spikes_are_counted_where_they_stand(slicer):
    n = 130
    corners = [(1, 1), (1, n - 2), (n - 2, 1), (n - 2, n - 2)]
    # both sides of every tile seam (rows 15 / 16, 31 / 32, 127 / 128, columns 63 / 64, 127 / 128); no two spikes touch
    seams = [(15, 40), (16, 44), (40, 63), (44, 64), (15, 63), (32, 64), (15, 127), (32, 128), (100, 127), (104, 128),
             (31, 5), (32, 9), (127, 63), (128, 70), (16, 60), (64, 128)]
    border = [(0, 5), (n - 1, 90), (9, 0), (70, n - 1), (0, 30), (n - 1, 20), (0, 64), (16, n - 1)]
    at = corners + seams + border
    H = len(at)
    edges = np.arange(H + 1, dtype=np.float64) + 0.5  # spike k alone in bin k; the zero background is below
    n_in = len(corners) + len(seams)
    by_hand = np.array([1] * n_in + [0] * len(border), np.int64)
    for sign, mine, other in ((1.0, "peaks", "minima"), (-1.0, "minima", "peaks")):
        x = spikes(n, at, sign)
        got = run(slicer, x, sign * edges[::-1] if sign < 0 else edges)
        hand = by_hand[::-1] if sign < 0 else by_hand
        assert np.array_equal(got[mine], hand), (sign, got[mine])
        assert not got[other].any() and not got["below"][1:].any() and not got["above"][1:].any()
        assert np.array_equal(got["pdf"], np.ones(H, np.int64))  # the border spikes are pixels all the same
        outside = got["below"][0] if sign > 0 else got["above"][0]
        assert outside == n * n - H and total(got) == n * n
        assert same(got, P.counts(x, got["edges"]))


def test_two_equal_adjacent_spikes_are_no_peaks(slicer):
    n = 130
    pairs = [((15, 20), (16, 20)), ((40, 63), (40, 64)), ((15, 127), (16, 128)), ((70, 70), (70, 71)), ((31, 63), (32, 64))]
    lone = (100, 100)
    edges = np.array([0.5, 1.5, 2.5])
    for sign in (1.0, -1.0):
        x = np.zeros((n, n), np.float32)
        for a, b in pairs:
            x[a] = x[b] = sign
        x[lone] = 2.0 * sign
        got = run(slicer, x, np.sort(sign * edges))
        mine, other = ("peaks", "minima") if sign > 0 else ("minima", "peaks")
        assert list(got[mine]) == ([0, 1] if sign > 0 else [1, 0])  # the lone spike only
        assert not got[other].any() and not got["below"][1:].any() and not got["above"][1:].any()
        assert list(got["pdf"]) == ([2 * len(pairs), 1] if sign > 0 else [1, 2 * len(pairs)])
    flat = run(slicer, np.full((n, n), 0.75, np.float32), edges)  # a plateau has no peaks
    assert not flat["peaks"].any() and not flat["minima"].any() and list(flat["pdf"]) == [n * n, 0]


def test_a_pixel_on_an_edge_is_in_the_bin_that_starts_there(slicer):
    f32 = np.float32
    edges = np.array([0.25, 0.5, 1.0, 2.0])  # all of them f32 values
    up = [np.nextafter(f32(e), f32(np.inf)) for e in edges]
    down = [np.nextafter(f32(e), f32(-np.inf)) for e in edges]
    x = np.full((8, 8), 0.75, f32)  # bin 1
    x[0, :4], x[1, :4], x[2, :4] = edges, up, down
    got = run(slicer, x, edges)
    # on the edges: bins 0, 1, 2 and the closed last bin 2; just above: 0, 1, 2, above; just below: below, 0, 1, 2
    assert list(got["pdf"]) == [1 + 1 + 1, 1 + 1 + 1 + 52, 2 + 1 + 1] and got["below"][0] == 1 and got["above"][0] == 1
    assert same(got, P.counts(x, edges))


def test_the_edges_are_compared_in_f64(slicer):
    f32 = np.float32
    x = f32(0.1)
    above_x, below_x = np.float64(x) * (1 + 2.0 ** -30), np.float64(x) * (1 - 2.0 ** -30)
    assert f32(above_x) == x == f32(below_x) and below_x < np.float64(x) < above_x  # rounded to f32 both edges are x
    m = np.full((5, 5), x, f32)
    for e, by_hand in ((above_x, [25, 0]), (below_x, [0, 25])):
        edges = np.array([0.0, e, 1.0])
        assert list(P.counts(m, edges)["pdf"]) == by_hand
        got = run(slicer, m, edges)
        assert list(got["pdf"]) == by_hand and got["below"][0] == got["above"][0] == 0
    # the same through the binary search's deeper levels
    for B in (7, 1024):
        edges = P.uniform_edges(0.0, 1.0, B)
        k = int(np.searchsorted(edges, np.float64(x)))
        for e, bin_of_x in ((above_x, k - 1), (below_x, k)):
            edges[k] = e
            got = run(slicer, m, edges)
            assert got["pdf"][bin_of_x] == 25 and got["pdf"].sum() == 25
            assert same(got, P.counts(m, edges))


def test_nan_and_infinite_pixels(slicer):
    n = 33
    x = make_map(n, "white").copy()
    nans, pinf, ninf = [(5, 5), (16, 16), (0, 3), (32, 32), (15, 31)], [(8, 20), (20, 8), (0, 0)], [(25, 25), (31, 1)]
    for at in nans:
        x[at] = np.nan
    for at in pinf:
        x[at] = np.inf
    for at in ninf:
        x[at] = -np.inf
    edges = P.uniform_edges(-1.0, 1.0, 7)
    got = check(slicer, x, edges)
    clean = make_map(n, "white")
    assert got["nan"] == len(nans)
    assert got["above"][0] == len(pinf) + int((clean > 1).sum()) - sum(clean[a] > 1 for a in nans + pinf + ninf)
    assert got["below"][0] == len(ninf) + int((clean < -1).sum()) - sum(clean[a] < -1 for a in nans + pinf + ninf)
    assert got["above"][1] >= 2 and got["below"][2] >= 2  # the interior infinities are a peak / a minimum each
    # a NaN's eight neighbours are neither: make every neighbour of one a would-be peak, then a would-be minimum
    for sign, name in ((1.0, "peaks"), (-1.0, "minima")):
        y = np.zeros((n, n), np.float32)
        y[10, 10] = np.nan
        y[9:12:2, 9:12:2] = sign  # the four diagonal neighbours: isolated spikes but for the NaN
        y[20, 20] = sign
        got = check(slicer, y, np.array([-1.5, -0.5, 0.5, 1.5]))
        assert got[name].sum() == 1 and got["nan"] == 1


@pytest.mark.parametrize("n", [64, 1024])
def test_an_input_off_the_16_byte_grid_gives_the_same_counts(slicer, n):
    x = make_map(n, "lognormal")
    edges = make_edges("lognormal", 64, "log")
    on, off = run(slicer, x, edges), run(slicer, x, edges, off_grid=True)
    assert same(on, off) and same(on, P.counts(x, edges, masks(n, "lognormal")))


def test_runs_repeat_and_carry_nothing_over(slicer):
    n = 257
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    edges = make_edges("white", 64, "uniform")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        with slicer_amd.Peaks(slicer, n, edges) as p:
            p.run(dx)
            first = p.read()
            p.run(dx)
            assert same(first, p.read())
            p.run(dy)  # a second, different map on the same handle
            second = p.read()
        assert same(first, P.counts(x, edges)) and same(second, run(slicer, y, edges))
        assert not same(first, second)
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def test_run_npix_on_a_smaller_map_is_a_handle_of_that_size(slicer):
    edges = make_edges("white", 64, "log")
    maps = {m: make_map(m, "white") for m in (200, 67, 64, 3, 1)}
    ptrs = {m: slicer.to_device(x) for m, x in maps.items()}
    try:
        with slicer_amd.Peaks(slicer, 200, edges) as p:
            for m in (200, 67, 64, 3, 1, 200):
                p.run(ptrs[m], m)
                got = p.read()
                assert same(got, run(slicer, maps[m], edges)) and total(got) == m * m
    finally:
        for d in ptrs.values():
            slicer.free(d)


@pytest.mark.parametrize("n", [66, 1000])
def test_run_level_over_a_moments_pyramid(slicer, n):
    x = make_map(n, "lognormal")
    levels = int(np.log2(n))
    edges = make_edges("lognormal", 64, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, levels) as m, slicer_amd.Peaks(slicer, n, edges) as p:
            m.run(d)
            p.run(d)
            assert same(p.read(), P.counts(x, edges))
            pyr = M.pyramid(x, levels, "mean")
            for level in range(1, levels + 1):
                p.run_level(m, level)
                got = p.read()
                y = m.read_map(level)
                assert y.tobytes() == pyr[level].tobytes()
                assert same(got, P.counts(y, edges)) and total(got) == (n >> level) ** 2
    finally:
        slicer.free(d)


def test_run_kappa_is_run_on_the_kappa_map(slicer):
    n = 48
    x = make_map(n, "lognormal")
    edges = make_edges("lognormal", 7, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Peaks(slicer, n, edges) as p:
            kappa.add_device([d], [[1.0]])
            p.run_kappa(kappa, 0)
            a = p.read()
            p.run(kappa.device_map(0))
            assert same(a, p.read()) and same(a, P.counts(kappa.read(0), edges))
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    edges = np.array([0.0, 1.0, 2.0])
    ph = C.c_void_p()
    assert L.slicer_peaks_create(slicer._h, n, 3, edges.ctypes.data, C.byref(ph)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.zeros(3, np.int64)
        assert L.slicer_peaks_read(ph, buf.ctypes.data, None, None, None, None, None) == ERR_STATE
        assert err() == "slicer_peaks_read before any slicer_peaks_run"
        assert L.slicer_peaks_run(ph, None) == ERR_ARG
        assert err() == "slicer_peaks_run: null argument"
        assert L.slicer_peaks_run_npix(ph, None, 4) == ERR_ARG
        assert err() == "slicer_peaks_run_npix: null argument"
        for bad in (0, -1, 17):
            assert L.slicer_peaks_run_npix(ph, d, bad) == ERR_ARG
            assert err() == f"slicer_peaks_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_peaks_read(ph, buf.ctypes.data, None, None, None, None, None) == ERR_STATE
        assert L.slicer_peaks_run(ph, d) == 0
        assert L.slicer_peaks_read(ph, buf.ctypes.data, None, None, None, None, None) == 0
        assert list(buf[:2]) == [n * n, 0]
        nan = C.c_int64(-1)
        assert L.slicer_peaks_read(ph, None, None, None, None, None, C.byref(nan)) == 0 and nan.value == 0
        out = C.c_void_p(1)
        assert L.slicer_peaks_create(slicer._h, n, 3, edges[::-1].copy().ctypes.data, C.byref(out)) == ERR_ARG
        assert err() == "slicer_peaks_create: edges must be strictly ascending"
        assert not out.value
        assert L.slicer_peaks_create(slicer._h, n, 3, edges.ctypes.data, None) == ERR_ARG
        assert err() == "slicer_peaks_create: null argument"
    finally:
        L.slicer_peaks_destroy(ph)
        slicer.free(d)
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Peaks(slicer, n, [0.0, np.nan])


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n, "white"))
    try:
        with slicer_amd.Peaks(slicer, n, make_edges("white", 7, "uniform")) as p:
            slicer.profile_reset()
            slicer.profile_enable(True)
            p.run(d)
            p.run(d, 32)
            p.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["peaks"][0] == 2 and prof["peaks_finish"][0] == 2
    finally:
        slicer.free(d)
