"""slicer_noise_* on the device.  The words are compared bit for bit with the host's; the maps with
the long double restatement tests/noise_np.py inside the contract's bound (K = 8) and its share condition; everything
else (two runs, load paths, pieces, sizes, layers) bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import noise_np as N
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 2, 3, 6
SEED = 0xFEDCBA9876543210
# the tail block with n^2 mod 4 = 0 and 1, under a workgroup (n^2 / 4 < 256), and many workgroups.  A square map never
# ends 2 or 3 pixels into a block: run_at does (test_a_run_that_ends_inside_a_block).  The threads stride only beyond
# kMaxGroups = 2^20 workgroups of 256 blocks of 4 pixels, a run of more than 2^30 pixels (n > 32768, 4 GiB of output):
# no test here reaches that loop's second round
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100, 257, 1000, 1024]
SIGMAS = (0.3, 1.0, 1e-3)


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=8)
def make_map(n, scale=1.0):
    x = (np.random.default_rng(6007 * n + 1).standard_normal(n * n) * scale).astype(np.float32)
    x.setflags(write=False)
    return x


def run(s, x, n, sigma, seed=SEED, stream=0, realisation=0, off=0):
    """read() of one run on a fresh handle; off: floats by which the input leaves the 16-byte grid."""
    d = None if x is None else s.to_device(np.concatenate([np.zeros(off, np.float32), x]))
    try:
        with slicer_amd.Noise(s, n, seed) as nz:
            nz.run(None if d is None else d + 4 * off, sigma, stream, realisation)
            return nz.read()
    finally:
        if d is not None:
            s.free(d)


def test_device_words_are_the_host_words(slicer):
    for seed, stream, real, first, count in ((0, 0, 0, 0, 4096), (SEED, 0xFFFFFFFF, 0x80000001, (1 << 32) - 8, 16),
                                             (1 << 63, 0x80000000, 0xFFFFFFFF, (1 << 63) + 5, 300),
                                             (0xFFFFFFFFFFFFFFFF, 7, 1 << 31, (1 << 64) - 4, 8)):
        with slicer_amd.Noise(slicer, 4, seed) as nz:
            got = nz.words(first, count, stream, real)
        blocks = [(first + k) % (1 << 64) for k in range(count)]
        want = np.stack([slicer_amd.noise_words(seed, stream, real, b) for b in blocks])
        assert got.dtype == np.uint32 and np.array_equal(got, want), (seed, first)
        assert np.array_equal(want, N.words(seed, stream, real, np.array(blocks, np.uint64)))


@pytest.mark.parametrize("n", SIZES)
def test_maps_are_inside_the_bound(slicer, n):
    for k, sigma in enumerate(SIGMAS):
        for x in (make_map(n), make_map(n, 1e10), None):
            got = run(slicer, x, n, sigma, stream=k, realisation=n)
            assert got.shape == (n, n) and got.dtype == np.float32
            ref, R = N.reference(x, sigma, SEED, k, n, count=n * n)
            ok, share, worst = N.check(got, ref, R, sigma)
            assert ok and share <= N.SHARE, (n, sigma, x is None, share, worst)
            if x is None:
                assert float(np.abs(got).max()) <= 6.77 * sigma and (n < 4 or float(got.std()) > 0)


def test_sigma_zero_returns_the_map(slicer):
    for n in (5, 64):
        x = make_map(n)
        assert np.array_equal(run(slicer, x, n, 0.0).ravel(), x)
    assert not run(slicer, None, 8, 0.0).any()


def test_nan_and_inf_stay_in_their_pixel(slicer):
    n = 33
    x = make_map(n).copy()
    special = {0: np.nan, 5: np.inf, 6: -np.inf, 514: np.nan, n * n - 1: -np.inf}
    clean = run(slicer, x, n, 0.3).ravel()
    for p, v in special.items():
        x[p] = v
    got = run(slicer, x, n, 0.3).ravel()
    others = np.ones(n * n, bool)
    for p, v in special.items():
        others[p] = False
        assert np.isnan(got[p]) if math.isnan(v) else got[p] == v
    assert got[others].tobytes() == clean[others].tobytes()


def test_the_hi_counter_word(slicer):
    """run_at with first_pixel >= 2^34: block >= 2^32, so the counter's second word is not 0."""
    x = make_map(8)
    for first in (1 << 34, (1 << 34) - 32, (1 << 63) + 4):
        d = slicer.to_device(x)
        try:
            with slicer_amd.Noise(slicer, 8, SEED) as nz:
                nz.run_at(d, first, 64, 1.0, 3, 4)
                got = nz.read()
                nz.run_at(None, first, 61, 1.0, 3, 4)
                pure = nz.read()
        finally:
            slicer.free(d)
        assert got.shape == (64,) and pure.shape == (61,)
        ref, R = N.reference(x, 1.0, SEED, 3, 4, first_pixel=first)
        ok, share, worst = N.check(got, ref, R, 1.0)
        assert ok and share == 0, (first, share, worst)
        ref, R = N.reference(None, 1.0, SEED, 3, 4, first_pixel=first, count=61)
        ok, share, worst = N.check(pure, ref, R, 1.0)
        assert ok and share == 0, (first, share, worst)
    assert not np.array_equal(got, run(slicer, x, 8, 1.0, stream=3, realisation=4).ravel())


def test_two_runs_are_equal_and_the_input_is_untouched(slicer):
    n = 100
    x = make_map(n)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Noise(slicer, n, SEED) as nz:
            nz.run(d, 0.3, 1, 2)
            a = nz.read()
            nz.run(d, 1.0, 9, 9)
            nz.run(d, 0.3, 1, 2)
            b = nz.read()
        assert np.array_equal(slicer.to_host(d, (n * n,), np.float32), x)
    finally:
        slicer.free(d)
    assert a.tobytes() == b.tobytes() == run(slicer, x, n, 0.3, stream=1, realisation=2).tobytes()


@pytest.mark.parametrize("n", [7, 64, 65, 257])
def test_both_load_paths_are_equal(slicer, n):
    """The handle owns its output, which therefore is always on the 16-byte grid; the input leaves it by 1, 2, 3 floats."""
    x = make_map(n)
    want = run(slicer, x, n, 0.3)
    for off in (1, 2, 3, 4):
        assert run(slicer, x, n, 0.3, off=off).tobytes() == want.tobytes(), off


@pytest.mark.parametrize("n,blocks", [(65, 4), (257, 1024), (100, 333), (9, 1)])
def test_pieces_are_one_run(slicer, n, blocks):
    x = make_map(n)
    want = run(slicer, x, n, 0.3, stream=2, realisation=1).ravel()
    want_pure = run(slicer, None, n, 0.3, stream=2, realisation=1).ravel()
    d = slicer.to_device(x)
    got, pure = [], []
    try:
        with slicer_amd.Noise(slicer, n, SEED) as nz:
            for first in range(0, n * n, 4 * blocks):
                count = min(4 * blocks, n * n - first)
                nz.run_at(d + 4 * first, first, count, 0.3, 2, 1)  # (a piece starts at a block, so on the 16-byte grid)
                got.append(nz.read())
                nz.run_at(None, first, count, 0.3, 2, 1)
                pure.append(nz.read())
    finally:
        slicer.free(d)
    assert np.concatenate(got).tobytes() == want.tobytes()
    assert np.concatenate(pure).tobytes() == want_pure.tobytes()


def test_a_smaller_map_is_the_start_of_a_larger_one(slicer):
    n = 65
    x = make_map(n)
    want = run(slicer, x, n, 0.3).ravel()
    d = slicer.to_device(x)
    try:
        with slicer_amd.Noise(slicer, n, SEED) as nz:
            for m in (1, 2, 17, 64):
                nz.run(d, 0.3, npix=m)
                got = nz.read()
                assert got.shape == (m, m) and got.tobytes() == want[:m * m].tobytes(), m
    finally:
        slicer.free(d)


def test_a_run_that_ends_inside_a_block(slicer):
    """count mod 4 = 1, 2, 3: the last block is loaded and stored pixel by pixel, on both load paths and without a map,
    and what it stores is the start of the whole block's values."""
    n = 9
    x = make_map(n)
    want = run(slicer, x, n, 0.3).ravel()
    want_pure = run(slicer, None, n, 0.3).ravel()
    d = slicer.to_device(np.concatenate([np.zeros(1, np.float32), x]))
    try:
        with slicer_amd.Noise(slicer, n, SEED) as nz:
            for count in (1, 2, 3, 5, 6, 7, 78, 79):
                for off in (1, 0):  # on the 16-byte grid and off it; x itself starts one float in
                    src = slicer.to_device(x[:count]) if off == 0 else None
                    try:
                        nz.run_at(d + 4 if src is None else src, 0, count, 0.3, 0, 0)
                        got = nz.read()
                    finally:
                        if src is not None:
                            slicer.free(src)
                    assert got.shape == (count,) and got.tobytes() == want[:count].tobytes(), (count, off)
                nz.run_at(None, 0, count, 0.3, 0, 0)
                assert nz.read().tobytes() == want_pure[:count].tobytes(), count
    finally:
        slicer.free(d)


def test_a_second_layer_in_place_is_two_handles_chained(slicer):
    n = 63
    x = make_map(n)
    d = slicer.to_device(x)
    try:
        with slicer_amd.Noise(slicer, n, SEED) as a, slicer_amd.Noise(slicer, n, SEED) as b:
            a.run(d, 0.3, 0, 0)
            b.run(a.device_map(), 0.5, 1, 0)
            chained = b.read()
            a.run(a.device_map(), 0.5, 1, 0)
            assert a.read().tobytes() == chained.tobytes()
            assert chained.tobytes() != run(slicer, x, n, 0.3).tobytes()
            # any other overlap with the own output is refused
            for shift in (4, 16, 4 * (n * n - 1)):
                assert L.slicer_noise_run(a._nh, a.device_map() + shift, 0.5, 0, 0) == ERR_ARG
                assert "overlaps" in (L.slicer_last_error(slicer._h) or b"").decode()
            assert L.slicer_noise_run_at(a._nh, a.device_map() - 16, 0, 8, 0.5, 0, 0) == ERR_ARG
            assert a.read().tobytes() == chained.tobytes()
    finally:
        slicer.free(d)


def test_run_kappa_and_run_level(slicer):
    n = 16
    planes = [slicer.to_device(make_map(n, 1.0 + k).reshape(n, n)) for k in range(2)]
    try:
        with slicer_amd.Kappa(slicer, n, 2) as kp, slicer_amd.Moments(slicer, n, 2) as mo, \
                slicer_amd.Noise(slicer, n, SEED) as nz:
            kp.add_device(planes, [[1.0, 0.5], [0.25, 2.0]])
            for s in range(2):
                kappa = kp.read(s)
                nz.run_kappa(kp, s, 0.3, s, 1)
                assert nz.read().tobytes() == run(slicer, kappa.ravel(), n, 0.3, stream=s, realisation=1).tobytes()
            mo.run_kappa(kp, 1)
            for level in (1, 2):
                x = mo.read_map(level)
                nz.run_level(mo, level, 0.3, 5, 6)
                got = nz.read()
                assert got.shape == x.shape == (n >> level, n >> level)
                assert got.tobytes() == run(slicer, x.ravel(), n >> level, 0.3, stream=5, realisation=6).tobytes()
    finally:
        for p in planes:
            slicer.free(p)


def test_refusals_and_state(slicer):
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    out = C.c_void_p(1)
    assert L.slicer_noise_create(slicer._h, 0, 0, C.byref(out)) == ERR_ARG and not out.value
    assert L.slicer_noise_create(slicer._h, 131073, 0, C.byref(out)) == ERR_UNSUPPORTED
    assert L.slicer_noise_create(slicer._h, 8, 0, None) == ERR_ARG
    d = slicer.to_device(make_map(8))
    host = np.zeros(64, np.float32)
    p = C.c_void_p()
    try:
        with slicer_amd.Noise(slicer, 8, 1) as nz:
            assert L.slicer_noise_read(nz._nh, host.ctypes.data) == ERR_STATE and "before any" in err()
            assert L.slicer_noise_device_map(nz._nh, C.byref(p)) == ERR_STATE
            for sigma in (-1.0, math.nan, math.inf):
                assert L.slicer_noise_run(nz._nh, d, sigma, 0, 0) == ERR_ARG and "sigma" in err()
            assert L.slicer_noise_run_npix(nz._nh, d, 0, 1.0, 0, 0) == ERR_ARG
            assert L.slicer_noise_run_npix(nz._nh, d, 9, 1.0, 0, 0) == ERR_ARG and "npix" in err()
            assert L.slicer_noise_run_at(nz._nh, d, 2, 4, 1.0, 0, 0) == ERR_ARG and "first_pixel" in err()
            assert L.slicer_noise_run_at(nz._nh, d, 0, 0, 1.0, 0, 0) == ERR_ARG
            assert L.slicer_noise_run_at(nz._nh, d, 0, 65, 1.0, 0, 0) == ERR_ARG and "count" in err()
            assert L.slicer_noise_words_device(nz._nh, 0, 0, 0, 0, d) == ERR_ARG
            assert L.slicer_noise_words_device(nz._nh, 0, 4, 0, 0, None) == ERR_ARG
            assert L.slicer_noise_read(nz._nh, host.ctypes.data) == ERR_STATE  # a refused run leaves no output
            nz.run(d, 1.0)
            assert L.slicer_noise_read(nz._nh, None) == ERR_ARG and L.slicer_noise_device_map(nz._nh, None) == ERR_ARG
            assert nz.read().shape == (8, 8) and nz.device_map()
    finally:
        slicer.free(d)


def test_both_kernels_are_in_the_profile(slicer):
    slicer.profile_reset()
    slicer.profile_enable(True)
    try:
        with slicer_amd.Noise(slicer, 16, 1) as nz:
            nz.run(None, 1.0)
            nz.run(None, 1.0)
            nz.words(0, 4)
            nz.read()
        slicer.synchronize()
        prof = slicer.profile_get()
    finally:
        slicer.profile_enable(False)
    assert prof["noise_add"][0] == 2 and prof["noise_words"][0] == 1
