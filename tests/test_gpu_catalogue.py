"""slicer_catalogue_* on the device against the restatement tests/catalogue_np.py.  Records are
compared byte for byte and counts as integers: nowhere a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

import catalogue_np as K
import peaks_np as P
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
INF = np.inf
# the sizes of tests/test_gpu_peaks.py: no interior (1, 2), one interior pixel (3), tile seams at rows 16 / 32 and columns
# 64 / 128, both load paths (4 | n or not)
SMALL = [1, 2, 3, 4, 5, 15, 16, 17, 18, 33, 63, 64, 65, 66, 67, 68, 100, 129]
MAPS = ("white", "lognormal", "integers")
POISON = 0xAB
GUARD = 64  # records behind a test's own buffer


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=8)
def make_map(n, kind, seed=0):
    rng = np.random.default_rng(104729 * n + seed)
    if kind == "integers":  # many ties
        x = rng.integers(-3, 4, (n, n))
    else:
        g = rng.standard_normal((n, n), np.float32)
        x = g if kind == "white" else np.exp(g) - np.float32(np.exp(0.5))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=8)
def reference(n, kind, seed=0):
    """Every peak and minimum of the map, computed once and left unchanged."""
    rec = K.catalogue(make_map(n, kind, seed))
    rec.setflags(write=False)
    return rec


def select(rec, kinds, min_peak, max_minimum):
    """The records of the full catalogue that a selection keeps (the selection changes no byte of a record)."""
    is_min = (rec["flags"] & K.MINIMUM).astype(bool)
    v = rec["value"].astype(np.float64)
    keep = np.where(is_min, bool(kinds & K.MINIMA) & (v <= max_minimum), bool(kinds & K.PEAKS) & (v >= min_peak))
    return rec[keep]


def selections(rec):
    """(min_peak, max_minimum, on a pixel): infinite thresholds, mid thresholds, and thresholds that are the values of a
    peak and of a minimum of the map -- the medians of each kind -- which pin >= and <= at equality."""
    is_min = (rec["flags"] & K.MINIMUM).astype(bool)
    pk, mn = rec["value"][~is_min].astype(np.float64), rec["value"][is_min].astype(np.float64)
    out = [(-INF, INF, False), (0.25, -0.25, False)]
    if len(pk) and len(mn):
        out.append((float(np.sort(pk)[len(pk) // 2]), float(np.sort(mn)[len(mn) // 2]), True))
    return out


def same_bytes(got, ref):
    assert got.dtype == K.DTYPE == lensing.CATALOGUE_DTYPE
    assert len(got) == len(ref), (len(got), len(ref))
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got != ref)[0]
        raise AssertionError((len(bad), got[bad[:3]], ref[bad[:3]]))


def check_run(cat, d, x, kinds, lo, hi, npix=None):
    ref = K.catalogue(x, kinds, lo, hi)
    cat.run(d, npix, kinds=kinds, min_peak=lo, max_minimum=hi)
    c = cat.counts()
    assert (c["peaks"], c["minima"]) == K.totals(ref) and c["stored"] == len(ref) and c["npix"] == x.shape[0]
    same_bytes(cat.read(), ref)
    return ref


@pytest.mark.parametrize("n", SMALL)
def test_records_are_the_restatement(slicer, n):
    counts = {}
    with slicer_amd.PeakCatalogue(slicer, n, n * n // 2 + 1) as cat:
        for kind in MAPS:
            x = make_map(n, kind)
            full = reference(n, kind)
            counts[kind] = len(full)
            d = slicer.to_device(x)
            try:
                for lo, hi, on_pixel in selections(full):
                    for kinds in (K.PEAKS, K.MINIMA, K.PEAKS | K.MINIMA):
                        ref = check_run(cat, d, x, kinds, lo, hi)
                        same_bytes(ref, select(full, kinds, lo, hi))
                    if on_pixel:  # a threshold on a pixel's value keeps that pixel
                        got = cat.read()
                        assert np.any((got["value"] == np.float32(lo)) & (got["flags"] & 1 == 0))
                        assert np.any((got["value"] == np.float32(hi)) & (got["flags"] & 1 == 1))
            finally:
                slicer.free(d)
    if n < 3:
        assert not any(counts.values())
    # Ties: of nine independent draws the centre is the strict maximum with probability 1 / 9 where values never repeat
    # and sum_v (1 / 7) (#values below v / 7)^8 = 0.053 on the seven integers: about half as many extrema.
    if n >= 33:
        assert counts["integers"] < 3 * counts["white"] // 4 and counts["white"] > (n - 2) ** 2 // 6


@pytest.mark.parametrize("n", [1425, 4096])
def test_records_of_large_maps_are_the_restatement(slicer, n):
    """1425: 90 x 23 = 2070 tiles with a short last tile row and column on the scalar path; 4096: 16384 tiles on the
    float4 path.  Both are more tiles than workgroups (at most 8 a CU) and more segments than one block of the scan
    (4096): 9 and 64 blocks."""
    x = make_map(n, "white")
    full = reference(n, "white")
    assert len(full) > (n - 2) ** 2 // 6
    d = slicer.to_device(x)
    try:
        with slicer_amd.PeakCatalogue(slicer, n, len(full) + 1) as cat:
            cat.run(d, kinds=K.PEAKS | K.MINIMA)
            c = cat.counts()
            assert (c["peaks"], c["minima"], c["stored"]) == K.totals(full) + (len(full),)
            same_bytes(cat.read(), full)
    finally:
        slicer.free(d)


@pytest.mark.parametrize("n", [64, 68, 129])
def test_a_map_off_the_16_byte_grid_gives_the_same_bytes(slicer, n):
    x = make_map(n, "lognormal")
    d_on = slicer.to_device(x)
    d_off = slicer.to_device(np.concatenate([np.zeros(1, np.float32), x.ravel()]))
    try:
        with slicer_amd.PeakCatalogue(slicer, n, n * n // 2) as cat:
            cat.run(d_on, kinds=3)
            on = cat.read()
            cat.run(d_off + 4, kinds=3)
            off = cat.read()
        same_bytes(on, reference(n, "lognormal"))
        same_bytes(off, on)
    finally:
        slicer.free(d_on)
        slicer.free(d_off)


def test_capacity_bounds_the_records_and_not_the_counts(slicer):
    n = 100
    x = make_map(n, "white")
    full = reference(n, "white")
    T = len(full)
    peaks, minima = K.totals(full)
    assert T > 1000 and peaks and minima
    d = slicer.to_device(x)
    try:
        for capacity in (T - 1, T, T + 1, 1):
            poison = np.full((capacity + GUARD) * 32, POISON, np.uint8)
            buf = slicer.to_device(poison)
            try:
                with slicer_amd.PeakCatalogue(slicer, n, capacity, d_records=buf) as cat:
                    cat.run(d, kinds=3)
                    c = cat.counts()
                    stored = min(T, capacity)
                    assert (c["peaks"], c["minima"], c["stored"]) == (peaks, minima, stored)
                    same_bytes(cat.read(), full[:stored])
                    for fewer in {0, 1, stored - 1} - {-1}:  # read with max_records < stored copies exactly that many
                        same_bytes(cat.read(fewer), full[:fewer])
                    same_bytes(cat.read(stored + 5), full[:stored])
                    d_rec, d_cnt = cat.device_records()
                    assert d_rec == buf
                    assert list(slicer.to_host(d_cnt, (3,), np.int64)) == [peaks, minima, stored]
                    raw = slicer.to_host(buf, poison.shape, np.uint8)
                assert raw[:stored * 32].tobytes() == full[:stored].tobytes()
                assert np.all(raw[stored * 32:] == POISON)  # the unused records and the guard behind the capacity
            finally:
                slicer.free(buf)
    finally:
        slicer.free(d)


@pytest.mark.parametrize("n,kind", [(67, "white"), (129, "lognormal"), (64, "integers"), (1425, "white")])
def test_counts_are_those_of_peaks_on_the_device(slicer, n, kind):
    x = make_map(n, kind)
    edges = P.uniform_edges(-1.0, 1.0, 7)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Peaks(slicer, n, edges) as p, slicer_amd.PeakCatalogue(slicer, n, 1) as cat:
            p.run(d)
            cat.run(d, kinds=3)
            r, c = p.read(), cat.counts()
        assert c["peaks"] == r["peaks"].sum() + r["below"][1] + r["above"][1]
        assert c["minima"] == r["minima"].sum() + r["below"][2] + r["above"][2]
        assert c["stored"] == min(1, c["peaks"] + c["minima"])
    finally:
        slicer.free(d)


def test_runs_repeat_and_carry_nothing_over(slicer):
    n = 130
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        with slicer_amd.PeakCatalogue(slicer, n, n * n // 2) as cat:
            first = check_run(cat, dx, x, 3, -INF, INF)
            cat.run(dx, kinds=3)
            same_bytes(cat.read(), first)  # the same bytes twice
            # another map, one kind, a high threshold: far fewer records -- stale counts or offsets would show
            second = check_run(cat, dy, y, K.PEAKS, 8.0, INF)
            assert 0 < len(second) < len(first) // 8
            c = cat.counts()
            assert c["minima"] == 0 and c["peaks"] == len(second)
            third = check_run(cat, dy, y, K.MINIMA, INF, -2.0)  # exp(g) - exp(0.5) > -1.65: an empty catalogue
            assert len(third) == 0 and cat.counts()["stored"] == 0
            check_run(cat, dx, x, 3, -INF, INF)
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def test_run_npix_and_run_level_over_a_moments_pyramid(slicer):
    n, levels = 132, 5
    x = make_map(n, "lognormal")
    d = slicer.to_device(x)
    small = {m: make_map(m, "white") for m in (67, 3, 1)}
    ptrs = {m: slicer.to_device(y) for m, y in small.items()}
    try:
        with slicer_amd.Moments(slicer, n, levels) as m, slicer_amd.PeakCatalogue(slicer, n, n * n // 2) as cat:
            m.run(d)
            check_run(cat, d, x, 3, -INF, INF)
            for level in range(1, levels + 1):
                y = m.read_map(level)
                ref = K.catalogue(y, 3, 0.0, 0.0)
                cat.run_level(m, level, kinds=3, min_peak=0.0, max_minimum=0.0)
                same_bytes(cat.read(), ref)
                assert cat.counts()["npix"] == n >> level and (len(ref) > 0 or n >> level < 8)
            for size, y in small.items():
                check_run(cat, ptrs[size], y, 3, -INF, INF, npix=size)
            check_run(cat, d, x, K.MINIMA, -INF, INF)
    finally:
        slicer.free(d)
        for p in ptrs.values():
            slicer.free(p)


def test_run_kappa_is_run_on_the_kappa_map(slicer):
    n = 48
    x = make_map(n, "lognormal")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.PeakCatalogue(slicer, n, n * n // 2) as cat:
            kappa.add_device([d], [[1.0]])
            cat.run_kappa(kappa, 0, kinds=3, min_peak=0.5)
            same_bytes(cat.read(), K.catalogue(kappa.read(0), 3, 0.5, INF))
    finally:
        slicer.free(d)


def test_every_class_of_the_refinement_on_the_device(slicer):
    """The hand-made windows of tests/test_catalogue_host.py, planted in one map away from each other, both signs: the
    device takes every branch of the refinement that the restatement takes, negative zeros included."""
    from test_catalogue_host import CLASSES, quadratic
    n = 70
    x = np.zeros((n, n), np.float32)
    at = [(2, 2), (2, 62), (2, 65), (14, 30), (17, 30), (40, 63), (40, 66)]
    for sign, shift in ((1.0, 0), (-1.0, 20)):
        for (i, j), (window, _, _) in zip(at, CLASSES.values()):
            x[i + shift - 1:i + shift + 2, j - 1:j + 2] = sign * np.asarray(window, np.float64)
    x[60:65, 10:15] = quadratic(5, (2, 2), 0.0, 0.0)  # offsets of -0.0
    ref, why = K.catalogue(x, with_why=True)
    assert {0, 1, 2, 4} <= set(why) and np.isinf(x).any() and np.isnan(x).any()
    assert np.any(np.signbit(ref["dy"]) & (ref["dy"] == 0.0)) and np.any(ref["flags"] & K.FALLBACK)
    d = slicer.to_device(x)
    try:
        with slicer_amd.PeakCatalogue(slicer, n, n * n // 2) as cat:
            cat.run(d, kinds=3)
            same_bytes(cat.read(), ref)
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    ch = C.c_void_p()
    assert L.slicer_catalogue_create(slicer._h, n, 8, None, C.byref(ch)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        k = C.c_int64(-1)
        for name, call in (("count", lambda: L.slicer_catalogue_count(ch, C.byref(k), None, None)),
                           ("read", lambda: L.slicer_catalogue_read(ch, None, 0, C.byref(k))),
                           ("device", lambda: L.slicer_catalogue_device(ch, None, None))):
            assert call() == ERR_STATE
            assert err() == f"slicer_catalogue_{name} before any slicer_catalogue_run"
        assert L.slicer_catalogue_run(ch, None, 1, 0.0, 0.0) == ERR_ARG
        assert err() == "slicer_catalogue_run: null argument"
        assert L.slicer_catalogue_run(ch, d, 4, 0.0, 0.0) == ERR_ARG
        assert err() == "slicer_catalogue_run: kinds = 4 outside 1..3"
        assert L.slicer_catalogue_run(ch, d, 1, np.nan, 0.0) == ERR_ARG
        assert err() == "slicer_catalogue_run: a threshold is NaN"
        for bad in (0, -1, 17):
            assert L.slicer_catalogue_run_npix(ch, d, 1, 0.0, 0.0, bad) == ERR_ARG
            assert err() == f"slicer_catalogue_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_catalogue_count(ch, C.byref(k), None, None) == ERR_STATE  # a refused run is no run
        assert L.slicer_catalogue_run(ch, d, 3, -INF, INF) == 0
        assert L.slicer_catalogue_count(ch, C.byref(k), None, None) == 0 and k.value == 0  # a flat map has none
        assert L.slicer_catalogue_read(ch, None, 4, None) == ERR_ARG
        assert err() == "slicer_catalogue_read: 4 records into a null array"
    finally:
        L.slicer_catalogue_destroy(ch)
        slicer.free(d)
    with slicer_amd.PeakCatalogue(slicer, n, 4) as cat:
        for call in (cat.counts, cat.read, cat.device_records):
            with pytest.raises(slicer_amd.SlicerError) as e:
                call()
            assert e.value.code == ERR_STATE
