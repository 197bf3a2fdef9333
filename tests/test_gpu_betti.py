"""slicer_betti_* on the device against the labelling of tests/betti_np.py (scipy.ndimage.label)
and against the Euler count of slicer_minkowski_* of the same map on the device.  Every count is an integer, so everything
here is exact: np.array_equal on int64, nowhere a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import betti_np as BT
import moments_np as M
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
# The kernels walk the flat map four (ranks) and eight (links) pixels a thread, so what matters is n^2 mod 4 and mod 8,
# maps that are all rim (1, 2), both parities, rows that are no multiple of 4, and more than one workgroup of 256
# threads (from n^2 > 1024 and 2048 on)
SMALL = [1, 2, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 67, 100, 129]
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


def run(s, x, thresholds, off_grid=False, euler=False):
    """read() of one run on a fresh handle; euler: also that of a Minkowski handle on the same device map."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Betti(s, n, thresholds) as b:
            b.run(d + 4 if off_grid else d)
            got = b.read()
        if euler:
            with slicer_amd.Minkowski(s, n, thresholds) as m:
                m.run(d + 4 if off_grid else d)
                mk = m.read()
            got["euler"], got["minkowski_faces"], got["minkowski_nan"] = mk["euler"], mk["faces"], mk["nan"]
        return got
    finally:
        s.free(d)


def check(s, x, thresholds, off_grid=False):
    got = run(s, x, thresholds, off_grid, euler=True)
    ref = BT.counts(x, thresholds)
    for k in BT.KEYS:
        assert np.array_equal(got[k], ref[k]), (x.shape[0], len(thresholds), k, got[k], ref[k])
    assert all(got[k].dtype == np.int64 and got[k].shape == (len(thresholds),) for k in BT.KEYS[:-1])
    assert np.array_equal(got["thresholds"], thresholds) and got["npix"] == x.shape[0]
    # the identity with N14's pixel complex, both sides from the device
    assert np.array_equal(got["components"] - got["holes"], got["euler"])
    assert np.array_equal(got["faces"], got["minkowski_faces"]) and got["nan"] == got["minkowski_nan"]
    return got


@pytest.mark.parametrize("n", SMALL)
def test_counts_are_the_labelling(slicer, n):
    for kind in KINDS:
        x = make_map(n, kind)
        for T in COUNTS:
            check(slicer, x, make_thresholds(kind, T, "log" if T == 8 else "uniform"))


def plateaus(n, seed):
    """Blocks of 8 x 8 equal integers, offset by 3: large plateaus, long equal-rank unions."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-3, 4, (n // 8 + 2, n // 8 + 2)).astype(np.float32)
    return np.kron(coarse, np.ones((8, 8), np.float32))[3:3 + n, 3:3 + n].copy()


# more workgroups than are resident (the grid-stride loops take several rounds) and, at 4096, more than 2^24 nodes.
# The labelling of either takes about a second on the host
@pytest.mark.parametrize("n,kind,thresholds", [
    (2048, "lognormal", make_thresholds("lognormal", 8, "uniform")),
    (4096, "plateaus", np.array([-0.5, 1.5])),
])
def test_counts_of_large_maps_are_the_labelling(slicer, n, kind, thresholds):
    x = plateaus(n, 1) if kind == "plateaus" else make_map(n, kind)
    got = check(slicer, x, thresholds)
    assert 0 < got["faces"][-1] < got["faces"][0] < n * n
    assert got["components"].min() > 1 and got["holes"].max() > 1


# ---- planted shapes at n = 130: 16900 pixels, 2113 groups of eight (the last one half empty), 9 workgroups ----
N = 130


def both_ways(s, x, want, want_flipped=None):
    """x holds zeros and ones: (components, holes) of {x >= 0.5} by hand and by the labelling, then the sign flipped and
    the threshold negated, whose set is the complement."""
    t = np.array([0.5])
    got = check(s, x, t)
    assert (int(got["components"][0]), int(got["holes"][0])) == want, got
    flipped = check(s, -x, -t[::-1])
    assert flipped["faces"][0] == N * N - got["faces"][0]
    if want_flipped is not None:
        assert (int(flipped["components"][0]), int(flipped["holes"][0])) == want_flipped, flipped


def test_planted_single_pixels(slicer):
    at = [(0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1),                      # corners
          (0, 5), (0, 63), (N - 1, 64), (9, 0), (120, 0), (70, N - 1),         # sides
          (15, 40), (16, 44), (64, 63), (65, 65), (127, 127), (2, 2), (128, 124)]  # interior
    H = len(at)
    t = np.arange(H, dtype=np.float64) + 0.5  # pixel k, of height k + 1, is in the sets 0 ... k
    x = np.zeros((N, N), np.float32)
    for k, a in enumerate(at):
        x[a] = 1.0 + k
    got = check(slicer, x, t)
    assert list(got["components"]) == list(range(H, 0, -1)) and not got["holes"].any()
    # flipped: the sets are the map without the pixels k ... H-1; those of them off the rim are holes
    flipped = check(slicer, -x, -t[::-1])
    inner = np.array([0 < i < N - 1 and 0 < j < N - 1 for i, j in at])
    assert np.all(flipped["components"] == 1)
    assert list(flipped["holes"]) == [int(inner[H - 1 - j:].sum()) for j in range(H)]


def test_planted_diagonal_chains(slicer):
    # the full diagonal: one component under 8-connectivity; its two sides are separate complement components and both
    # reach the rim.  Flipped: the sides join across the diagonal's corners, and every diagonal pixel off the rim is a hole
    x = np.eye(N, dtype=np.float32)
    both_ways(slicer, x, (1, 0), (1, N - 2))
    # short chains in both directions, an L of them, and a closed diamond (one hole, the 4-connected inside)
    x = np.zeros((N, N), np.float32)
    for k in range(20):
        x[5 + k, 60 + k] = 1        # down-right across column 63 / 64
        x[100 - k, 10 + k] = 1      # up-right
    for k in range(6):              # a diamond of diagonals around (50, 100)
        x[50 - 6 + k, 100 + k] = x[50 + k, 100 + 6 - k] = x[50 + 6 - k, 100 - k] = x[50 - k, 100 - 6 + k] = 1
    both_ways(slicer, x, (3, 1))


def test_planted_checkerboard(slicer):
    x = (np.add.outer(np.arange(N), np.arange(N)) % 2 == 0).astype(np.float32)
    inside = (N - 2) * (N - 2) // 2  # the empty squares off the rim; flipped, the full ones
    both_ways(slicer, x, (1, inside), (1, inside))


def test_planted_rings_and_rim_pockets(slicer):
    x = np.zeros((N, N), np.float32)
    rings = [(16, 64), (32, 127), (48, 63), (127, 127), (80, 20)]  # centres of 3 x 3 rings: one component, one hole each
    for ci, cj in rings:
        x[ci - 1:ci + 2, cj - 1:cj + 2] = 1
        x[ci, cj] = 0
    # a ring inside a ring: a hole that holds a component that holds a hole
    x[95:110, 95:110] = 1
    x[96:109, 96:109] = 0
    x[99:106, 99:106] = 1
    x[102, 102] = 0
    # a ring cut open by the rim: its pocket pixel lies on the first row, so it is no hole
    x[0, 30], x[0, 32] = 1, 1
    x[1, 30:33] = 1
    # a pocket closed by pixels that themselves lie on the rim: the empty pixel (N - 2, 1) touches no rim
    x[N - 3:, 0:3] = 1
    x[N - 2, 1] = 0
    both_ways(slicer, x, (len(rings) + 4, len(rings) + 3))
    # the same as heights: every shape leaves the sets one after the other
    t = np.arange(4, dtype=np.float64) + 0.5
    y = x.copy()
    y[95:110, 95:110] *= 2   # both nested rings
    y[99:106, 99:106] *= 2   # the inner one: height 4
    y[0:2, 30:33] *= 3
    got = check(slicer, y, t)
    assert list(got["components"]) == [9, 3, 2, 1] and list(got["holes"]) == [8, 2, 1, 1]
    check(slicer, -y, -t[::-1])


def spiral(n):
    """A one-pixel-wide square spiral from (0, 0) inwards with one-pixel gaps."""
    x = np.zeros((n, n), np.float32)
    i = j = 0
    di, dj = 0, 1
    x[0, 0] = 1

    def ahead(di, dj):  # the next cell is free, and the one after it is not part of the path
        a, b, a2, b2 = i + di, j + dj, i + 2 * di, j + 2 * dj
        if not (0 <= a < n and 0 <= b < n) or x[a, b]:
            return False
        return not (0 <= a2 < n and 0 <= b2 < n and x[a2, b2])

    while True:
        if not ahead(di, dj):
            di, dj = dj, -di  # turn right
            if not ahead(di, dj):
                return x
        i, j = i + di, j + dj
        x[i, j] = 1


def serpentine(n):
    """Every other row of the map's inside, joined at alternating ends."""
    x = np.zeros((n, n), np.float32)
    for k, r in enumerate(range(1, n - 1, 2)):
        x[r, 1:n - 1] = 1
        if r + 2 < n - 1:
            x[r + 1, n - 2 if k % 2 == 0 else 1] = 1
    return x


def test_planted_spiral_and_serpentine(slicer):
    # the longest parent chains: one component of more than 8000 pixels each; the complement is one component that
    # reaches the rim.  Flipped: the gaps are one component too; the serpentine, off the rim, is its one hole
    s, z = spiral(N), serpentine(N)
    assert s.sum() > 8000 and z.sum() > 8000
    both_ways(slicer, s, (1, 0), (1, 0))
    both_ways(slicer, z, (1, 0), (1, 1))
    both_ways(slicer, s.T.copy(), (1, 0), (1, 0))
    both_ways(slicer, z[::-1, ::-1].T.copy(), (1, 0), (1, 1))


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
    # the thresholds are compared in f64: a threshold that rounds to the pixel's f32 value from above excludes it
    v = f32(0.1)
    m = np.full((5, 5), v, f32)
    for thr, faces in ((np.float64(v) * (1 + 2.0 ** -30), 0), (np.float64(v) * (1 - 2.0 ** -30), 25)):
        got = check(slicer, m, np.array([thr]))
        assert got["faces"][0] == faces and got["components"][0] == (1 if faces else 0) and got["holes"][0] == 0


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
    assert got["faces"][-1] >= len(pinf) and got["components"][-1] >= 1  # +inf is in every set
    # enclosed NaN pixels are holes at every threshold, NaN pixels on the rim never; +inf is in every set
    y = np.full((n, n), np.inf, np.float32)
    for at in nans:
        y[at] = np.nan
    walled = check(slicer, y, t)
    assert np.all(walled["components"] == 1) and np.all(walled["holes"] == 3) and np.all(walled["faces"] == n * n - 6)
    assert walled["nan"] == 6
    # a map of NaN and -inf alone is in no set
    y = np.full((n, n), np.nan, np.float32)
    y[::2] = -np.inf
    empty = check(slicer, y, t)
    assert not any(empty[k].any() for k in BT.KEYS[:-1]) and empty["nan"] == int(np.isnan(y).sum())
    # a flat map: one component without a hole below its rank, nothing above
    flat = np.full((n, n), 0.25, np.float32)
    for T in (1, 8, 1025):
        thr = make_thresholds("integers", T, "uniform")
        got = check(slicer, flat, thr)
        k = int(np.searchsorted(thr, 0.25, "right"))
        assert k >= 1 and np.all(got["components"][:k] == 1) and not got["components"][k:].any() and not got["holes"].any()


@functools.lru_cache(maxsize=1)
def speckled_map():
    """White noise of 67^2 = 4489 pixels -- the last quad of k_betti_rank holds one pixel, which the float4 kernel loads
    on its scalar path -- with a few NaN, +inf and -inf pixels, that last pixel among them."""
    x = make_map(67, "white").copy()
    x[3, 5] = x[40, 66] = x[66, 66] = np.nan
    x[0, 0] = x[30, 31] = np.inf
    x[66, 0] = x[12, 60] = -np.inf
    x.setflags(write=False)
    return x


# k_betti_rank keeps its T + 1 u32 rank counters in 2^c copies, c the largest <= 5 with 4 (T + 1) 2^c <= 16384 B (lg_copies
# of slicer_rank_counts.hpp): 32 copies up to T = 127, 16 up to 255, 8 up to 511, 4 up to 1023, 2 above.  The last and the
# first T of every count; the fold of the copies at the flush has to give the counts of one copy.
@pytest.mark.parametrize("T", [127, 128, 255, 256, 511, 512, 1023, 1024, 1025])
def test_counts_at_every_number_of_counter_copies(slicer, T):
    x = speckled_map()
    t = make_thresholds("white", T, "uniform")
    got, ref = run(slicer, x, t), BT.counts(x, t)
    for k in BT.KEYS:
        assert np.array_equal(got[k], ref[k]), (T, k, got[k], ref[k])
    assert got["nan"] == 3 and got["faces"][0] > got["faces"][-1] >= 2


@pytest.mark.parametrize("n", [64, 129])
def test_an_input_off_the_16_byte_grid_gives_the_same_counts(slicer, n):
    x = make_map(n, "lognormal")
    t = make_thresholds("lognormal", 65, "log")
    on, off = run(slicer, x, t), run(slicer, x, t, off_grid=True)
    assert BT.same(on, off) and BT.same(on, BT.counts(x, t))


def test_runs_repeat_and_carry_nothing_over(slicer):
    n = 257
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    t = make_thresholds("white", 65, "uniform")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        with slicer_amd.Betti(slicer, n, t) as b:
            b.run(dx)
            first = b.read()
            b.run(dx)
            assert BT.same(first, b.read())
            b.run(dy)  # a second, different map on the same handle
            second = b.read()
        assert BT.same(first, BT.counts(x, t)) and BT.same(second, run(slicer, y, t))
        assert not BT.same(first, second)
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def test_run_npix_on_a_smaller_map_is_a_handle_of_that_size(slicer):
    t = make_thresholds("white", 65, "log")
    maps = {m: make_map(m, "white") for m in (200, 67, 64, 3, 1)}
    ptrs = {m: slicer.to_device(x) for m, x in maps.items()}
    try:
        with slicer_amd.Betti(slicer, 200, t) as b:
            for m in (200, 67, 64, 3, 1, 200):
                b.run(ptrs[m], m)
                got = b.read()
                assert BT.same(got, BT.counts(maps[m], t)) and got["npix"] == m
                assert BT.same(got, run(slicer, maps[m], t))
    finally:
        for d in ptrs.values():
            slicer.free(d)


def test_run_level_over_a_moments_pyramid(slicer):
    n = 66
    x = make_map(n, "lognormal")
    levels = int(np.log2(n))
    t = make_thresholds("lognormal", 65, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, levels) as m, slicer_amd.Betti(slicer, n, t) as b:
            m.run(d)
            b.run(d)
            assert BT.same(b.read(), BT.counts(x, t))
            pyr = M.pyramid(x, levels, "mean")
            for level in range(1, levels + 1):
                b.run_level(m, level)
                got = b.read()
                y = m.read_map(level)
                assert y.tobytes() == pyr[level].tobytes()
                assert BT.same(got, BT.counts(y, t)) and got["npix"] == n >> level
    finally:
        slicer.free(d)


def test_run_kappa_is_run_on_the_kappa_map(slicer):
    n = 48
    x = make_map(n, "lognormal")
    t = make_thresholds("lognormal", 8, "uniform")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Betti(slicer, n, t) as b:
            kappa.add_device([d], [[1.0]])
            b.run_kappa(kappa, 0)
            a = b.read()
            b.run(kappa.device_map(0))
            assert BT.same(a, b.read()) and BT.same(a, BT.counts(kappa.read(0), t))
            assert a["faces"][0] > a["faces"][-1] > 0 and a["components"][0] > 0
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.ones(n * n, np.float32))
    t = np.array([0.0, 1.0, 2.0])
    bh = C.c_void_p()
    assert L.slicer_betti_create(slicer._h, n, 3, t.ctypes.data, C.byref(bh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.zeros(3, np.int64)
        assert L.slicer_betti_read(bh, buf.ctypes.data, None, None, None) == ERR_STATE
        assert err() == "slicer_betti_read before any slicer_betti_run"
        assert L.slicer_betti_run(bh, None) == ERR_ARG
        assert err() == "slicer_betti_run: null argument"
        assert L.slicer_betti_run_npix(bh, None, 4) == ERR_ARG
        assert err() == "slicer_betti_run_npix: null argument"
        for bad in (0, -1, 17):
            assert L.slicer_betti_run_npix(bh, d, bad) == ERR_ARG
            assert err() == f"slicer_betti_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_betti_read(bh, buf.ctypes.data, None, None, None) == ERR_STATE
        assert L.slicer_betti_run(bh, d) == 0
        assert L.slicer_betti_read(bh, buf.ctypes.data, None, None, None) == 0
        assert list(buf) == [1, 1, 0]
        faces, nan = np.zeros(3, np.int64), C.c_int64(-1)
        assert L.slicer_betti_read(bh, None, buf.ctypes.data, faces.ctypes.data, C.byref(nan)) == 0
        assert list(buf) == [0, 0, 0] and list(faces) == [n * n, n * n, 0] and nan.value == 0
        assert L.slicer_betti_read(bh, None, None, None, None) == 0
        out = C.c_void_p(1)
        assert L.slicer_betti_create(slicer._h, n, 3, t[::-1].copy().ctypes.data, C.byref(out)) == ERR_ARG
        assert err() == "slicer_betti_create: thresholds must be strictly ascending"
        assert not out.value
        assert L.slicer_betti_create(slicer._h, n, 3, t.ctypes.data, None) == ERR_ARG
        assert err() == "slicer_betti_create: null argument"
    finally:
        L.slicer_betti_destroy(bh)
        slicer.free(d)
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Betti(slicer, n, [0.0, np.nan])
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Betti(slicer, n, [])
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.Betti(slicer, slicer_amd.BETTI_MAX_NPIX + 1, [0.0])


def test_the_kernels_show_in_the_profile(slicer):
    # per run: one betti_rank (the ranks and their column sums), two betti_link (the set sweep; the parents' reset with
    # the complement sweep) and one betti_finish
    n = 64
    d = slicer.to_device(make_map(n, "white"))
    try:
        with slicer_amd.Betti(slicer, n, make_thresholds("white", 8, "uniform")) as b:
            slicer.profile_reset()
            slicer.profile_enable(True)
            b.run(d)
            b.run(d, 32)
            b.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["betti_rank"][0] == 2 and prof["betti_link"][0] == 4 and prof["betti_finish"][0] == 2
    finally:
        slicer.free(d)
