"""Host side of the binned power spectra: the numpy restatement (tests/power_np.py) against a
brute-force loop, analytic fields, white noise and smr.PS's bin list, and slicer_power_bins against the restatement.
No GPU needed."""
import math

import numpy as np
import pytest

import power_np
import shear_np
import slicer_amd
from slicer_amd import lensing


def brute_force(kappa, angle, edges):
    """One Python loop over the half plane, straight from the contract."""
    n = kappa.shape[0]
    khat = np.fft.rfft2(kappa.astype(np.float64))
    e2 = [float(r) * float(r) for r in edges]
    B = len(edges) - 1
    cnt, rs, ps = [0] * B, [0.0] * B, [0.0] * B
    for i0 in range(n):
        j0 = i0 if i0 < (n + 1) // 2 else i0 - n
        for j1 in range(n // 2 + 1):
            m2 = j0 * j0 + j1 * j1
            for b in range(B):
                if e2[b] <= m2 < e2[b + 1] or (b == B - 1 and m2 == e2[B]):
                    cnt[b] += 1
                    rs[b] += math.sqrt(m2)
                    ps[b] += abs(khat[i0, j1]) ** 2
                    break
    theta = math.radians(angle)
    cl = [theta ** 2 / n ** 4 * p / c if c else math.nan for c, p in zip(cnt, ps)]
    mean = [r / c if c else math.nan for c, r in zip(cnt, rs)]
    return np.array(cnt), np.array(mean), np.array(cl)


def brute_force_cross(spectra, angle, edges):
    """Every pair of the half-plane spectra ([n][n // 2 + 1] each) by the same loop: -> counts [B], cl [S][S][B], scale
    [S][S][B] (theta^2 / n^4 times the bin mean of |khat_s| |khat_t|).  The terms of a bin are summed with math.fsum,
    so the sums carry no error of their own beyond the rounding of each product."""
    S, n = len(spectra), spectra[0].shape[0]
    khat = np.stack(spectra)
    e2 = [float(r) * float(r) for r in edges]
    B = len(edges) - 1
    terms = [[] for _ in range(B)]
    mags = [[] for _ in range(B)]
    for i0 in range(n):
        j0 = i0 if i0 < (n + 1) // 2 else i0 - n
        for j1 in range(n // 2 + 1):
            m2 = j0 * j0 + j1 * j1
            for b in range(B):
                if e2[b] <= m2 < e2[b + 1] or (b == B - 1 and m2 == e2[B]):
                    x = khat[:, i0, j1]
                    terms[b].append(np.outer(x.real, x.real) + np.outer(x.imag, x.imag))
                    mags[b].append(np.outer(np.abs(x), np.abs(x)))
                    break
    norm = math.radians(angle) ** 2 / n ** 4
    cnt = np.array([len(t) for t in terms])
    cl, scale = np.full((S, S, B), np.nan), np.full((S, S, B), np.nan)
    for b in range(B):
        if cnt[b]:
            t, m = np.stack(terms[b]), np.stack(mags[b])
            for s in range(S):
                for u in range(s, S):
                    cl[s, u, b] = cl[u, s, b] = norm * (math.fsum(t[:, s, u]) / cnt[b])
                    scale[s, u, b] = scale[u, s, b] = norm * (math.fsum(m[:, s, u]) / cnt[b])
    return cnt, cl, scale


@pytest.mark.parametrize("n", [3, 6, 15, 16])
def test_restatement_of_pairs_matches_brute_force(n):
    rng = np.random.default_rng(70 + n)
    maps = [rng.standard_normal((n, n)) * (1.0 + s) for s in range(4)]
    for edges in (power_np.default_edges(n), [0.5, 1.0, 2.0, 2.5, 5.0]):
        cnt, cl, scale = brute_force_cross([np.fft.rfft2(m) for m in maps], 3.0, edges)
        ref = power_np.power(maps, 3.0, edges, cross=True)
        assert np.array_equal(ref["counts"], cnt)
        assert np.array_equal(np.isnan(cl), np.isnan(ref["cl"]))
        nz = cnt > 0
        assert np.all(np.abs(cl - ref["cl"])[..., nz] <= 1e-13 * scale[..., nz])
        np.testing.assert_allclose(scale[..., nz], ref["scale"][..., nz], rtol=1e-12)
        for s in range(4):  # the diagonal is the single-map loop above
            np.testing.assert_allclose(cl[s, s], brute_force(maps[s], 3.0, edges)[2], rtol=1e-12, equal_nan=True)


@pytest.mark.parametrize("n", [2, 3, 6, 7, 8, 12, 15])
def test_restatement_matches_brute_force(n):
    rng = np.random.default_rng(n)
    kappa = rng.standard_normal((n, n))
    for edges in (power_np.default_edges(n), [0.5, 1.0, 2.0, 2.5, 5.0], [0.0, 1.0, math.sqrt(2.0), 3.0]):
        cnt, mean, cl = brute_force(kappa, 3.0, edges)
        ref = power_np.power([kappa], 3.0, edges)
        assert np.array_equal(ref["counts"], cnt)
        np.testing.assert_allclose(ref["cl"][0], cl, rtol=1e-12, equal_nan=True)
        c2, m2 = power_np.bins(n, edges)
        assert np.array_equal(c2, cnt)
        np.testing.assert_allclose(m2, mean, rtol=1e-14, equal_nan=True)


@pytest.mark.parametrize("n,a,b", [(16, 3, 0), (16, 5, 0), (30, 2, 5), (45, 4, 7), (16, 1, 2), (32, 6, 8)])
def test_restatement_on_analytic_cosines(n, a, b):
    """kappa = A cos(2 pi (a i0 + b i1) / n), 0 < a, b < n / 2: its rfft2 is A n^2 / 2 at (a, b) alone when b > 0, and
    at (a, 0) and (-a, 0) when b = 0 -- both of radius a, in the same bin.  So the bin of sqrt(a^2 + b^2) holds
    theta^2 / n^4 * (number of such coefficients) * (A n^2 / 2)^2 / N_b and every other bin 0."""
    angle, A = 4.0, 0.3
    theta = math.radians(angle)
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    kappa = A * np.cos(2 * np.pi * (a * i0 + b * i1) / n)
    ref = power_np.power([kappa], angle)
    cl, counts = ref["cl"][0], ref["counts"]
    r = math.sqrt(a * a + b * b)
    home = int(math.floor(r))  # default edges: bin k holds k <= radius < k + 1
    coeffs = 1 if b > 0 else 2
    expect = theta ** 2 / n ** 4 * coeffs * (A * n * n / 2) ** 2 / counts[home]
    assert cl[home] == pytest.approx(expect, rel=1e-12)
    others = np.delete(cl, home)
    assert np.all(np.abs(others[np.isfinite(others)]) <= 1e-20 * expect)


def test_default_edges_are_smr_ps_bins():
    """smr.PS: kf = min(KX[1, 0], KY[0, 1]) with K = 2 pi fftfreq(n, size / n); bins = [i * kf for i in range(n)]."""
    for n, angle in ((16, 5.0), (1000, 5.0), (4096, 10.0)):
        size = math.radians(angle)
        kx = 2 * np.pi * np.fft.fftfreq(n, size / n)
        ky = 2 * np.pi * np.fft.rfftfreq(n, size / n)
        kf = min(kx[1], ky[1])
        smr_bins = np.array([i * kf for i in range(n)])
        ours = power_np.default_edges(n) * lensing.ell_fundamental(angle)
        assert ours.size == n
        np.testing.assert_allclose(ours, smr_bins, rtol=1e-14)
        assert lensing.ell_fundamental(angle) == power_np.ell_f(angle)


def test_white_noise_gives_the_pixel_solid_angle():
    n, angle, sigma = 128, 2.0, 1.7
    theta = math.radians(angle)
    kappa = np.random.default_rng(3).standard_normal((n, n)) * sigma
    khat = np.fft.rfft2(kappa)
    ref = power_np.power_of_spectra([khat], angle)
    cl, counts = ref["cl"][0], ref["counts"]
    ok = counts > 0
    mean = float((cl[ok] * counts[ok]).sum() / counts[ok].sum())
    per_mode = theta ** 2 / n ** 4 * np.abs(khat) ** 2
    err = per_mode.std() / math.sqrt(per_mode.size)
    expect = sigma ** 2 * theta ** 2 / n ** 2
    assert abs(mean - expect) < 5 * err, (mean, expect, err)


def log_edges(n):
    return np.concatenate([[0.0], np.geomspace(1.0, n * 0.75, 24)])


@pytest.mark.parametrize("n", [2, 3, 16, 30, 45, 4096, 16384])
def test_power_bins_match_the_restatement(n):
    edge_sets = [None, log_edges(n), np.array([0.0, 2.0, 5.0, 7.5, 25.0, 30.0])]
    for edges in edge_sets:
        got = slicer_amd.power_bins(n, edges)
        cnt, mean = power_np.bins(n, edges)
        assert np.array_equal(got["counts"], cnt), edges
        assert np.array_equal(np.isnan(got["mean_radius"]), cnt == 0)
        ok = cnt > 0
        rel = np.abs(got["mean_radius"][ok] - mean[ok]) / mean[ok].clip(min=1e-300)
        assert np.all((rel <= 1e-13) | (mean[ok] == 0)), float(rel.max())
    if n >= 16:  # a mode of exactly radius 5 and 25 (3-4-5, 7-24-25, 15-20-25) sits on the upper edge's side
        got = slicer_amd.power_bins(n, [0.0, 5.0, 25.0])["counts"]
        cnt, _ = power_np.bins(n, [0.0, 5.0, 25.0])
        assert np.array_equal(got, cnt)


def test_power_bins_counts_every_mode_once():
    for n in (15, 16, 49):
        got = slicer_amd.power_bins(n)["counts"]
        assert got.sum() == n * (n // 2 + 1)  # the default edges reach radius n - 1 > n / sqrt(2)


@pytest.mark.parametrize("edges", [[0.0], [], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("inf")],
                                   [0.0, float("nan"), 3.0]])
def test_power_bins_refuses_bad_edges(edges):
    with pytest.raises(slicer_amd.SlicerError) as e:
        slicer_amd.power_bins(16, np.array(edges, np.float64))
    assert e.value.code == 2  # SLICER_ERR_ARG


def test_power_bins_refuses_bad_sizes_and_default_length():
    L = lensing._L
    c = np.zeros(16, np.int64)
    m = np.zeros(16)
    assert L.slicer_power_bins(0, 2, np.array([0.0, 1.0]).ctypes.data, c.ctypes.data, m.ctypes.data) == 2
    assert L.slicer_power_bins(16, 15, None, c.ctypes.data, m.ctypes.data) == 2  # default edges: n_edges = npix
    assert L.slicer_power_bins(16, 16, None, None, m.ctypes.data) == 2
    assert b"npix" in L.slicer_last_error(None) or b"null" in L.slicer_last_error(None)


def test_ell_edges_are_divided_by_the_fundamental():
    n_edges, e = lensing._edges(64, None, [100.0, 200.0, 400.0], 5.0)
    assert n_edges == 3
    np.testing.assert_array_equal(e, np.array([100.0, 200.0, 400.0]) / lensing.ell_fundamental(5.0))
    with pytest.raises(ValueError):
        lensing._edges(64, [0.0, 1.0], [1.0, 2.0], 5.0)


def test_clustered_maps_have_a_red_spectrum():
    """Sanity of the restatement on the maps the GPU tests use: smoothing moves power to large scales."""
    n = 64
    ref = power_np.power([shear_np.clustered(n, 1)], 5.0)
    cl = ref["cl"][0]
    assert cl[1:4].mean() > cl[40:44].mean()
