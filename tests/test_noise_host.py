"""The shape-noise contract without a device: Philox4x32-10's known answers from the restatement
tests/noise_np.py and from slicer_noise_words; the statistics of the restated normals; that the bound tells an f32
evaluation from an f64 one; slicer_noise_sigma_pix and slicer_smooth_noise_gain; the refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import noise_np as N
import slicer_amd
import smooth_np as S
from slicer_amd import lensing

L = lensing._L
LD = np.longdouble
ERR_ARG, ERR_UNSUPPORTED = 2, 6
# Random123's published vectors (kat_vectors, philox4x32 10): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
COUNT = 1 << 22


def _err():
    return (L.slicer_last_error(None) or b"").decode()


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answers(counter, key, want):
    assert N.philox(*counter, *key).tolist() == list(want)
    # counter (lo b, hi b, realisation, stream), key (lo seed, hi seed)
    block, seed = counter[0] | counter[1] << 32, key[0] | key[1] << 32
    assert N.words(seed, counter[3], counter[2], block).tolist() == list(want)
    assert slicer_amd.noise_words(seed, counter[3], counter[2], block).tolist() == list(want)


def test_the_library_words_are_the_restatement():
    rng = np.random.default_rng(13)
    n = 10000
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    stream = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    real = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    block = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    block[::3] >>= np.uint64(40)  # small ones too
    block[1::7] = (np.uint64(1) << np.uint64(32)) + np.arange(block[1::7].size, dtype=np.uint64) - np.uint64(4)
    assert int((block >= 1 << 32).sum()) > 1000 and int((block < 1 << 32).sum()) > 1000
    want = N.words(seed, stream, real, block)
    got = np.stack([slicer_amd.noise_words(int(s), int(t), int(r), int(b)) for s, t, r, b in zip(seed, stream, real, block)])
    assert got.dtype == want.dtype == np.uint32 and np.array_equal(got, want)


@pytest.fixture(scope="module")
def fields():
    """Restated normals of COUNT pixels, f64 copies: the base and one with another stream, realisation and seed each."""
    base = dict(seed=0x1234567890ABCDEF, stream=3, realisation=5)
    out = {"base": N.field(base["seed"], base["stream"], base["realisation"], 0, COUNT)[0].astype(np.float64)}
    for what, other in (("seed", base["seed"] + 1), ("stream", 4), ("realisation", 6)):
        a = dict(base)
        a[what] = other
        out[what] = N.field(a["seed"], a["stream"], a["realisation"], 0, COUNT)[0].astype(np.float64)
    return out


def test_the_normals_are_standard_normals(fields):
    """Within 5 sampling sigma: Var(mean) = 1 / n, Var(m2) = 2 / n, Var(m3) = 15 / n, Var(m4) = (105 - 9) / n."""
    z = fields["base"]
    n = z.size
    assert float(np.abs(z).max()) <= 6.77
    assert abs(z.mean()) <= 5 * math.sqrt(1 / n)
    assert abs((z ** 2).mean() - 1) <= 5 * math.sqrt(2 / n)
    assert abs((z ** 3).mean()) <= 5 * math.sqrt(15 / n)
    assert abs((z ** 4).mean() - 3) <= 5 * math.sqrt(96 / n)


def test_the_normals_are_uncorrelated(fields):
    """A product of two independent standard normals has variance 1, so a mean over m of them has the sigma 1 / sqrt(m)."""
    z = fields["base"]
    lanes = z.reshape(-1, 4)
    m = lanes.shape[0]
    for a in range(4):
        for b in range(a + 1, 4):
            assert abs((lanes[:, a] * lanes[:, b]).mean()) <= 5 / math.sqrt(m), (a, b)
    assert abs((z[:-1] * z[1:]).mean()) <= 5 / math.sqrt(z.size - 1)  # adjacent pixels
    assert abs((z[:-2048] * z[2048:]).mean()) <= 5 / math.sqrt(z.size - 2048)  # adjacent rows of a 2048^2 map
    for what in ("seed", "stream", "realisation"):
        assert abs((z * fields[what]).mean()) <= 5 / math.sqrt(z.size), what


def test_seed_stream_and_realisation_each_change_the_map(fields):
    base = fields["base"].astype(np.float32)
    for what in ("seed", "stream", "realisation"):
        assert np.count_nonzero(fields[what].astype(np.float32) != base) > 0.99 * base.size, what


def test_the_field_does_not_depend_on_where_a_run_starts():
    z, R = N.field(7, 1, 2, 0, 1000)
    for first, count in ((0, 17), (4, 996), (512, 488), (996, 3)):
        z1, R1 = N.field(7, 1, 2, first, count)
        assert np.array_equal(z1, z[first:first + count]) and np.array_equal(R1, R[first:first + count])


@pytest.mark.parametrize("with_x", [True, False])
def test_the_bound_tells_an_f32_evaluation_from_an_f64_one(with_x):
    n, sigma, seed = 256, 0.3, 99
    x = np.random.default_rng(5).standard_normal(n * n).astype(np.float32) if with_x else None
    ref, R = N.reference(x, sigma, seed, 2, 1, count=n * n)
    ok, share, worst = N.check(N.emulate(x, sigma, seed, 2, 1, n * n, np.float64), ref, R, sigma)
    assert ok and share <= N.SHARE, (share, worst)
    ok, share, worst = N.check(N.emulate(x, sigma, seed, 2, 1, n * n, np.float32), ref, R, sigma)
    assert not ok or share > N.SHARE, (share, worst)
    assert share > 0.25  # (an f32 evaluation misses the rounded reference in most pixels)


def test_sigma_pix_is_the_formula():
    for sigma_e, ngal, angle, npix in ((0.26, 30.0, 2.0, 32), (0.3, 8.5, 3.5, 4096), (0.4, 0.1, 10.0, 30), (0.26, 30.0, 5.0, 131072)):
        side = np.float64(60.0) * np.float64(angle) / np.float64(npix)
        want = np.float64(sigma_e) / np.sqrt(np.float64(ngal) * (side * side))
        got = slicer_amd.noise_sigma_pix(sigma_e, ngal, angle, npix)
        assert got == float(want)
        exact = LD(sigma_e) / np.sqrt(LD(ngal) * (LD(60) * LD(angle) / LD(npix)) ** 2)
        assert abs(LD(got) - exact) <= 4 * LD(2.0) ** -53 * exact
    # per component: 0.26 and 30 galaxies per arcmin^2 on 1-arcmin pixels
    assert abs(slicer_amd.noise_sigma_pix(0.26, 30.0, 1.0, 60) - 0.26 / math.sqrt(30.0)) < 1e-15


def weights_2d(kind, sigma, t=4.0):
    """The (2R+1)^2 weights of an interior output pixel, long double, from the library's tables."""
    R, g, h = slicer_amd.smooth_weights(sigma, t)
    g = np.concatenate([g[:0:-1], g]).astype(LD)
    h = np.concatenate([h[:0:-1], h]).astype(LD)
    if kind == "gauss":
        return R, np.outer(g, g) / g.sum() ** 2
    c = 1 / (2 * N.PI_LD * LD(sigma) * LD(sigma))
    return R, c * (np.outer(g, g) - np.outer(h, g) - np.outer(g, h))


@pytest.mark.parametrize("kind", ["gauss", "map"])
@pytest.mark.parametrize("sigma", [1.5, 3.0])
def test_noise_gain(kind, sigma):
    n = 257
    gain = slicer_amd.smooth_noise_gain(kind, sigma)
    R, W = weights_2d(kind, sigma)
    brute = np.sqrt((W * W).sum())
    assert abs(LD(gain) - brute) <= 1e-13 * brute
    # against the rms of the restatement of N12 applied to restated unit noise, over the pixels at least R from the edges
    z = N.field(2024, 0, 0, 0, n * n)[0].astype(np.float32).reshape(n, n)
    _, g, h = slicer_amd.smooth_weights(sigma)
    y = S.smooth(kind, z, g, h, sigma).astype(np.float64)[R:n - R, R:n - R]
    rms = math.sqrt((y * y).mean())
    # The smoothed pixels are correlated with rho = (W * W) / sum W^2, the filter's autocorrelation.  For a Gaussian field
    # Var(mean y^2) = 2 s^4 sum_pq rho_pq^2 / m^2 <= 2 s^4 sum_d rho(d)^2 / m, so the rms has the relative sigma
    # sqrt(1 / (2 m_eff)), m_eff = m / sum_d rho(d)^2: the effective sample count (about 3900, 960 for gauss at 1.5, 3).
    m = y.size
    pad = np.zeros((4 * R + 2, 4 * R + 2))
    pad[:2 * R + 1, :2 * R + 1] = W.astype(np.float64)
    auto = np.fft.irfft2(np.abs(np.fft.rfft2(pad)) ** 2, pad.shape)
    rho = auto / auto[0, 0]
    m_eff = m / float((rho * rho).sum())
    assert 100 < m_eff < m
    assert abs(rms / gain - 1) <= 5 * math.sqrt(1 / (2 * m_eff)), (rms, gain, m_eff)


def test_noise_gain_truncate():
    for kind in ("gauss", "map"):
        R, W = weights_2d(kind, 2.0, 5.0)
        assert R == 10
        brute = np.sqrt((W * W).sum())
        assert abs(LD(slicer_amd.smooth_noise_gain(kind, 2.0, 5.0)) - brute) <= 1e-13 * brute
    # a wide Gaussian: 1 / (4 pi s^2) per unit variance, up to the truncation
    assert abs(slicer_amd.smooth_noise_gain("gauss", 8.0, 8.0) ** 2 * 4 * math.pi * 64 - 1) < 1e-6


def test_refusals_that_need_no_device():
    out = C.c_double(-1.0)
    ok = (0.26, 30.0, 2.0, 32)
    for k, bad in [(k, b) for k in range(3) for b in (0.0, -1.0, math.nan, math.inf, -math.inf)] + [(3, 0), (3, -5)]:
        a = list(ok)
        a[k] = bad
        assert L.slicer_noise_sigma_pix(a[0], a[1], a[2], a[3], C.byref(out)) == ERR_ARG, (k, bad)
        assert "slicer_noise_sigma_pix" in _err() and out.value == -1.0
    assert L.slicer_noise_sigma_pix(*ok, None) == ERR_ARG
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.noise_sigma_pix(0.26, 0.0, 2.0, 32)
    assert L.slicer_noise_words(0, 0, 0, 0, None) == ERR_ARG

    for kind, sigma, t, code in ((2, 1.0, 4.0, ERR_ARG), (-1, 1.0, 4.0, ERR_ARG), (0, 0.0, 4.0, ERR_ARG),
                                 (0, math.nan, 4.0, ERR_ARG), (1, 1.0, 0.5, ERR_ARG), (1, 1.0, 9.0, ERR_ARG),
                                 (0, 0.1, 4.0, ERR_ARG), (1, 32.125, 4.0, ERR_UNSUPPORTED)):
        assert L.slicer_smooth_noise_gain(kind, sigma, t, C.byref(out)) == code, (kind, sigma, t)
        assert _err() and out.value == -1.0
    assert L.slicer_smooth_noise_gain(0, 1.0, 4.0, None) == ERR_ARG
    with pytest.raises(ValueError):
        slicer_amd.smooth_noise_gain("tophat", 1.0)

    nh = C.c_void_p(1)
    assert L.slicer_noise_create(None, 0, 0, C.byref(nh)) == ERR_ARG and "npix" in _err() and not nh.value
    assert L.slicer_noise_create(None, -3, 0, C.byref(nh)) == ERR_ARG
    assert L.slicer_noise_create(None, 131073, 0, C.byref(nh)) == ERR_UNSUPPORTED and "131072" in _err()
    assert L.slicer_noise_create(None, 131072, 0, C.byref(nh)) == ERR_ARG and "null" in _err()
    for sigma in (-1e-300, -1.0, math.nan, math.inf, -math.inf):
        assert L.slicer_noise_run(None, None, sigma, 0, 0) == ERR_ARG and "sigma" in _err()
        assert L.slicer_noise_run_npix(None, None, 4, sigma, 0, 0) == ERR_ARG and "sigma" in _err()
        assert L.slicer_noise_run_at(None, None, 0, 4, sigma, 0, 0) == ERR_ARG and "sigma" in _err()
    for first in (1, 2, 3, 5, (1 << 40) + 2):
        assert L.slicer_noise_run_at(None, None, first, 4, 1.0, 0, 0) == ERR_ARG and "first_pixel" in _err()
    assert L.slicer_noise_run(None, None, 1.0, 0, 0) == ERR_ARG and "null" in _err()
    assert L.slicer_noise_run_at(None, None, 4, 4, 0.0, 0, 0) == ERR_ARG and "null" in _err()
    assert L.slicer_noise_words_device(None, 0, 0, 0, 0, None) == ERR_ARG and "n_blocks" in _err()
    assert L.slicer_noise_words_device(None, 0, (1 << 32) + 1, 0, 0, None) == ERR_ARG and "n_blocks" in _err()
    assert L.slicer_noise_words_device(None, 0, 1, 0, 0, None) == ERR_ARG and "null" in _err()
    assert L.slicer_noise_device_map(None, None) == ERR_ARG and L.slicer_noise_read(None, None) == ERR_ARG
    assert L.slicer_noise_destroy(None) == ERR_ARG
