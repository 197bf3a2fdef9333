"""slicer_smooth_* on the device against the restatement tests/smooth_np.py fed with the library's
own tables (smooth_weights).  Everything is compared as values (==) with equal NaN positions: nowhere a tolerance."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import moments_np as M
import slicer_amd
import smooth_np as S
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 2, 3, 6
KINDS = ("gauss", "map")
# R >= n, the row kernel's seams (rows 4 k, column 256), the column kernel's (columns 32 k and 64 k, rows 48 k and 64 k for
# the tiles that cols_cfg picks at these scales), both load paths (4 | n or not)
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 47, 48, 49, 63, 64, 65, 66, 67, 68, 95, 96, 97, 100, 127, 128, 129, 191,
         192, 193, 239, 240, 241, 255, 256, 257, 260]
SCALES = (0.3, 1.0, 2.5, 8.0, 32.0)  # at truncate 4: R = 1, 4, 10, 32 and the limit 128


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=4)
def make_map(n, kind="lognormal", seed=0):
    rng = np.random.default_rng(7919 * n + seed)
    g = rng.standard_normal((n, n), np.float32)
    x = (g if kind == "white" else np.exp(g) - np.float32(math.exp(0.5))).astype(np.float32)
    x.setflags(write=False)
    return x


def restate(kind, x, sigma, t=4.0):
    _, g, h = slicer_amd.smooth_weights(sigma, t)
    return S.smooth(kind, x, g, h, sigma)


def same(got, ref):
    """Equal values and equal NaN positions (the sign of a zero and NaN payloads carry no contract)."""
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and bool(
        np.all((got == ref) | (np.isnan(got) & np.isnan(ref))))


def run(s, kind, x, sigma, t=4.0, off_grid=False):
    """read() of one run on a fresh handle."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Smooth(s, n, kind, sigma, t) as sm:
            sm.run(d + 4 if off_grid else d)
            return sm.read()
    finally:
        s.free(d)


def check(s, kind, x, sigma, t=4.0):
    got = run(s, kind, x, sigma, t)
    ref = restate(kind, x, sigma, t)
    if not same(got, ref):
        bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
        raise AssertionError((kind, x.shape[0], sigma, t, int(bad.sum()), np.argwhere(bad)[:4].tolist()))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_maps_are_the_restatement(slicer, n):
    for mapkind in ("white", "lognormal"):
        x = make_map(n, mapkind)
        for sigma in SCALES:
            for kind in KINDS:
                check(slicer, kind, x, sigma)


@pytest.mark.parametrize("n,sigma,kind", [(n, sg, k) for n in (1000, 1023, 1024) for sg in (2.5, 13.7) for k in KINDS] +
                         [(2048, 4.0, "gauss"), (2048, 4.0, "map"), (4096, 1.0, "map")])
def test_large_maps_are_the_restatement(slicer, n, sigma, kind):
    got = check(slicer, kind, make_map(n), sigma)
    assert np.isfinite(got).all() and float(np.abs(got).max()) > 0


@pytest.mark.parametrize("sigma,t", [(2.0, 1.0), (7.3, 1.0), (2.5, 5.0), (13.7, 5.0), (1.0, 8.0), (5.1, 8.0), (16.0, 8.0),
                                     (128.0, 1.0)])
def test_truncate(slicer, sigma, t):
    R = int(t * sigma + 0.5)
    assert 1 <= R <= 128
    for n in (33, 100):
        for kind in KINDS:
            with slicer_amd.Smooth(slicer, n, kind, sigma, t) as sm:
                assert sm.radius == R
            check(slicer, kind, make_map(n), sigma, t)


def test_radius_128_is_taken_and_129_refused(slicer):
    for sigma, t in ((32.0, 4.0), (16.06, 8.0), (128.4, 1.0)):
        with slicer_amd.Smooth(slicer, 8, "map", sigma, t) as sm:
            assert sm.radius == 128
    out = C.c_void_p(1)
    for sigma, t in ((32.125, 4.0), (16.07, 8.0), (128.5, 1.0)):
        assert L.slicer_smooth_create(slicer._h, 8, 0, sigma, t, C.byref(out)) == ERR_UNSUPPORTED
        assert "moments pyramid" in (L.slicer_last_error(slicer._h) or b"").decode() and not out.value


@pytest.mark.parametrize("n", [5, 65, 130])
def test_a_constant_map_stays_constant_under_gauss(slicer, n):
    one = np.ones((n, n), np.float32)
    for sigma in SCALES:
        got = run(slicer, "gauss", one, sigma)
        assert got.tobytes() == one.tobytes(), (n, sigma)
    assert (run(slicer, "gauss", np.float32(-2.5) * one, 2.5) == np.float32(-2.5)).all()


# (row, column) in a map of 300: the corners, both sides of the row kernel's seams (rows 3 | 4, columns 255 | 256) and of
# the column kernel's (columns 31 | 32, 63 | 64, rows 47 | 48, 63 | 64, 95 | 96, 127 | 128, 191 | 192, 239 | 240, 255 | 256)
SPIKES = [(0, 0), (0, 299), (299, 0), (299, 299), (3, 255), (4, 256), (3, 256), (4, 255), (47, 31), (48, 32), (63, 63),
          (64, 64), (95, 64), (96, 63), (127, 128), (128, 127), (191, 255), (192, 256), (150, 150), (299, 256), (239, 15),
          (240, 16), (255, 16), (256, 15)]


@pytest.mark.parametrize("sigma", [1.0, 2.5, 8.0])
def test_a_unit_spike_reaches_its_window_and_nothing_else(slicer, sigma):
    n = 300
    R, g, h = slicer_amd.smooth_weights(sigma)
    for kind in KINDS:
        with slicer_amd.Smooth(slicer, n, kind, sigma) as sm:
            assert sm.radius == R
            for i, j in SPIKES:
                x = np.zeros((n, n), np.float32)
                x[i, j] = 1.0
                d = slicer.to_device(x)
                try:
                    sm.run(d)
                    got = sm.read()
                finally:
                    slicer.free(d)
                inside = np.zeros((n, n), bool)
                inside[max(i - R, 0):i + R + 1, max(j - R, 0):j + R + 1] = True
                assert not got[~inside].any(), (kind, sigma, i, j)
                # a radius that is too small would leave zeros on the window's rim: g_R g_R and U there are not zero
                rim = [(a, b) for a in (i - R, i + R) for b in (j - R, j + R) if 0 <= a < n and 0 <= b < n]
                assert rim and all(got[a, b] != 0 for a, b in rim), (kind, sigma, i, j)
                assert same(got, S.smooth(kind, x, g, h, sigma)), (kind, sigma, i, j)


@pytest.mark.parametrize("sigma", [1.0, 2.5])
def test_nan_and_inf_reach_exactly_their_windows(slicer, sigma):
    n = 33
    clean = make_map(n)
    x = clean.copy()
    at_nan, at_inf = (5, 20), (25, 3)
    x[at_nan], x[at_inf] = np.nan, np.inf
    R = slicer_amd.smooth_weights(sigma)[0]
    window = np.zeros((n, n), bool)
    nan_window = np.zeros((n, n), bool)
    for (i, j), w in ((at_nan, nan_window), (at_inf, window)):
        w[max(i - R, 0):i + R + 1, max(j - R, 0):j + R + 1] = True
    window |= nan_window
    for kind in KINDS:
        before = run(slicer, kind, clean, sigma)
        got = check(slicer, kind, x, sigma)
        assert np.array_equal(~np.isfinite(got), window), kind
        assert np.isnan(got[nan_window]).all()
        assert got[~window].tobytes() == before[~window].tobytes()  # every other output keeps its bits


@pytest.mark.parametrize("n", [64, 1024])
def test_an_input_off_the_16_byte_grid_gives_the_same_map(slicer, n):
    x = make_map(n)
    for kind in KINDS:
        on, off = run(slicer, kind, x, 2.5), run(slicer, kind, x, 2.5, off_grid=True)
        assert on.tobytes() == off.tobytes() and same(on, restate(kind, x, 2.5))


def test_runs_repeat_and_carry_nothing_over(slicer):
    n = 257
    x, y = make_map(n, "white"), make_map(n, "lognormal")
    dx, dy = slicer.to_device(x), slicer.to_device(y)
    try:
        for kind in KINDS:
            with slicer_amd.Smooth(slicer, n, kind, 2.5) as sm:
                sm.run(dx)
                first = sm.read()
                sm.run(dx)
                assert sm.read().tobytes() == first.tobytes()
                sm.run(dy)  # a second, different map on the same handle
                second = sm.read()
            assert same(first, restate(kind, x, 2.5)) and second.tobytes() == run(slicer, kind, y, 2.5).tobytes()
            assert first.tobytes() != second.tobytes()
        assert slicer.to_host(dx, (n, n), np.float32).tobytes() == x.tobytes()  # the input is untouched
    finally:
        slicer.free(dx)
        slicer.free(dy)


def test_run_npix_on_a_smaller_map_is_a_handle_of_that_size(slicer):
    maps = {m: make_map(m) for m in (200, 67, 64, 3, 1)}
    ptrs = {m: slicer.to_device(x) for m, x in maps.items()}
    try:
        for kind in KINDS:
            with slicer_amd.Smooth(slicer, 200, kind, 2.5) as sm:
                for m in (200, 67, 64, 3, 1, 200, 3, 67):  # smaller after larger and back
                    sm.run(ptrs[m], m)
                    got = sm.read()
                    assert got.shape == (m, m) and got.tobytes() == run(slicer, kind, maps[m], 2.5).tobytes(), (kind, m)
    finally:
        for d in ptrs.values():
            slicer.free(d)


def test_run_level_over_a_moments_pyramid(slicer):
    n = 66
    x = make_map(n)
    levels = int(np.log2(n))
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, levels) as m:
            m.run(d)
            pyr = M.pyramid(x, levels, "mean")
            for kind in KINDS:
                with slicer_amd.Smooth(slicer, n, kind, 1.0) as sm:
                    sm.run(d)
                    assert same(sm.read(), restate(kind, x, 1.0))
                    for level in range(1, levels + 1):
                        sm.run_level(m, level)
                        y = m.read_map(level)
                        assert y.tobytes() == pyr[level].tobytes()
                        got = sm.read()
                        assert got.shape == y.shape and same(got, restate(kind, y, 1.0)), (kind, level)
    finally:
        slicer.free(d)


def test_run_kappa_and_a_second_handle_on_a_smoothed_map(slicer):
    n = 48
    x = make_map(n)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Smooth(slicer, n, "gauss", 1.5) as a, \
                slicer_amd.Smooth(slicer, n, "map", 2.5) as b:
            kappa.add_device([d], [[1.0]])
            a.run_kappa(kappa, 0)
            first = a.read()
            assert same(first, restate("gauss", kappa.read(0), 1.5))
            b.run(a.device_map(), n)  # the smoothed map, where it is
            assert same(b.read(), restate("map", first, 2.5))
            assert a.read().tobytes() == first.tobytes()
            # a handle does not take its own output as its input
            assert L.slicer_smooth_run(a._sh, a.device_map()) == ERR_ARG
            assert "overlaps" in (L.slicer_last_error(slicer._h) or b"").decode()
            assert L.slicer_smooth_run_npix(a._sh, a.device_map() + 4 * n * n - 4, 1) == ERR_ARG
            assert a.read().tobytes() == first.tobytes()
    finally:
        slicer.free(d)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    sh = C.c_void_p()
    assert L.slicer_smooth_create(slicer._h, n, 1, 2.0, 4.0, C.byref(sh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.zeros((n, n), np.float32)
        p = C.c_void_p()
        assert L.slicer_smooth_read(sh, buf.ctypes.data) == ERR_STATE
        assert err() == "slicer_smooth_read before any slicer_smooth_run"
        assert L.slicer_smooth_device_map(sh, C.byref(p)) == ERR_STATE
        assert err() == "slicer_smooth_device_map before any slicer_smooth_run"
        assert L.slicer_smooth_run(sh, None) == ERR_ARG and err() == "slicer_smooth_run: null argument"
        assert L.slicer_smooth_run_npix(sh, None, 4) == ERR_ARG and err() == "slicer_smooth_run_npix: null argument"
        for bad in (0, -1, 17):
            assert L.slicer_smooth_run_npix(sh, d, bad) == ERR_ARG
            assert err() == f"slicer_smooth_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_smooth_read(sh, buf.ctypes.data) == ERR_STATE
        assert L.slicer_smooth_run(sh, d) == 0
        assert L.slicer_smooth_read(sh, None) == ERR_ARG and L.slicer_smooth_device_map(sh, None) == ERR_ARG
        assert L.slicer_smooth_read(sh, buf.ctypes.data) == 0 and not buf.any()
        assert L.slicer_smooth_device_map(sh, C.byref(p)) == 0 and p.value
        out = C.c_void_p(1)
        assert L.slicer_smooth_create(slicer._h, n, 7, 2.0, 4.0, C.byref(out)) == ERR_ARG and not out.value
        assert L.slicer_smooth_create(slicer._h, n, 0, 0.1, 4.0, C.byref(out)) == ERR_ARG and "radius 0" in err()
        assert L.slicer_smooth_create(slicer._h, n, 0, 2.0, 4.0, None) == ERR_ARG
        assert err() == "slicer_smooth_create: null argument"
    finally:
        L.slicer_smooth_destroy(sh)
        slicer.free(d)
    for bad in (dict(sigma_pix=math.nan), dict(sigma_pix=2.0, truncate=0.5), dict(sigma_pix=40.0)):
        with pytest.raises(slicer_amd.SlicerError):
            slicer_amd.Smooth(slicer, n, "gauss", **bad)


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n))
    try:
        with slicer_amd.Smooth(slicer, n, "gauss", 2.5) as a, slicer_amd.Smooth(slicer, n, "map", 2.5) as b:
            slicer.profile_reset()
            slicer.profile_enable(True)
            a.run(d)
            a.run(d, 32)
            b.run(d)
            a.read()
            b.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["smooth_rows"][0] == 3 and prof["smooth_cols"][0] == 3 and prof["smooth_norm"][0] == 2
    finally:
        slicer.free(d)
