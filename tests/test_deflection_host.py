"""The restatement tests/deflection_np.py against answers taken by hand; no GPU."""
import numpy as np
import pytest

import deflection_np as dn
import shear_np


def grid(n):
    return np.meshgrid(np.arange(n, dtype=np.longdouble), np.arange(n, dtype=np.longdouble), indexing="ij")


@pytest.mark.parametrize("n", [5, 6, 9, 17])
def test_d2_is_exact_on_cubics_and_quadratics_edges_included(n):
    """The reference's own (never invoked) test_laplacian_03: the one-sided four-point formula is exact on cubics too."""
    i, j = grid(n)
    c = 3
    for axis in (0, 1):
        assert np.array_equal(dn.d2((i + j - c) ** 3, 1.0, axis), 6 * (i + j - c))
        assert np.array_equal(dn.d2((i + j - c) ** 2, 2.0, axis), np.full((n, n), 0.5, np.longdouble))


@pytest.mark.parametrize("n", [5, 8, 13])
def test_d1_is_exact_on_quartics_in_the_interior(n):
    i, j = grid(n)
    d = 0.5
    x, y = i * d, j * d
    f = (x - 1) ** 4 - 2 * x ** 3 + x * y ** 3 + y ** 4
    g0 = dn.d1(f, d, 0)[2:-2]
    g1 = dn.d1(f, d, 1)[:, 2:-2]
    ref0 = (4 * (x - 1) ** 3 - 6 * x ** 2 + y ** 3)[2:-2]
    ref1 = (3 * x * y ** 2 + 4 * y ** 3)[:, 2:-2]
    scale = float(np.abs(f).max()) / d
    assert float(np.abs(g0 - ref0).max()) <= 1e-17 * scale
    assert float(np.abs(g1 - ref1).max()) <= 1e-17 * scale
    # and the edge samples are the plain two-point differences
    assert np.array_equal(dn.d1(f, d, 0)[0], (f[1] - f[0]) / np.longdouble(d))
    assert np.array_equal(dn.d1(f, d, 0)[-2], (f[-2] - f[-3]) / np.longdouble(d))


@pytest.mark.parametrize("n", [5, 7, 33])
def test_mixed_derivative_commutes(n):
    phi = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
    m = dn.fd_maps(phi, 0.25)
    assert float(np.abs(m["p12"] - m["p21"]).max()) <= 8 * 2.0 ** -63 * float(np.abs(m["p12"]).max())
    # the device evaluates p12 alone: the contract's (p12 + p21) / 2 is the same number to the reference's own rounding
    assert float(np.abs(m["gamma2"] - m["p12"]).max()) <= 8 * 2.0 ** -63 * float(np.abs(m["p12"]).max())


def test_rescale_is_a_second_spacing():
    phi = dn.noise_on_one(9, 1)
    a, b = dn.rescale(dn.fd_maps(phi, 1.0), 1.0, 0.003), dn.fd_maps(phi, 0.003)
    for k in dn.FD_NAMES:
        assert float(np.abs(a[k] - b[k]).max()) <= 2.0 ** -60 * float(np.abs(b[k]).max()), k


@pytest.mark.parametrize("n,a,b", [(64, 3, 2), (64, -3, 2), (45, 2, 5), (100, -4, 3)])
def test_single_cosine_mode(n, a, b):
    """kappa = A cos(x), x = 2 pi (a i0 + b i1) / n: phi = -2 kappa / k^2, alpha_a = 2 A K_a sin(x) / k^2.  The stencils
    on the exact phi: D1 e^{ikx} = ik (1 - (kd)^4 / 30 + ...) e^{ikx}, D2 e^{ikx} = -k^2 (1 - (kd)^4 / 90 + ...) e^{ikx},
    both series alternating, so the leading term bounds the truncation error and is nearly attained."""
    angle, A = 4.0, 0.7
    theta = np.deg2rad(angle)
    d = theta / n
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = 2 * np.pi * ((a * i0 + b * i1) % n) / n
    K0, K1 = 2 * np.pi * a / theta, 2 * np.pi * b / theta
    k2 = K0 * K0 + K1 * K1
    kappa, phi = A * np.cos(x), -2 * A * np.cos(x) / k2
    exact = {"alpha1": 2 * A * K0 * np.sin(x) / k2, "alpha2": 2 * A * K1 * np.sin(x) / k2}
    got = dn.deflection(kappa, angle)
    for k, g in zip(("alpha1", "alpha2"), got):
        assert np.abs(g - exact[k]).max() <= 1e-12 * np.abs(exact[k]).max(), k
    fd = dn.fd_maps(phi, d)
    inner = (slice(2, -2), slice(2, -2))
    for k, K in (("alpha1", K0), ("alpha2", K1)):
        lead = (abs(K) * d) ** 4 / 30 * np.abs(exact[k]).max()
        err = float(np.abs(fd[k] - exact[k])[inner].max())
        assert 0.8 * lead <= err <= lead * (1 + 1e-9), (k, err, lead)
    g1 = shear_np.shear(kappa, angle)["gamma1"]
    lead = 0.5 * (K0 ** 6 + K1 ** 6) * d ** 4 / 90 * np.abs(phi).max()
    err = float(np.abs(fd["gamma1"] - g1)[inner].max())
    assert err <= lead * (1 + 1e-6) + 1e-12 * np.abs(g1).max(), (err, lead)
    assert err >= 0.5 * abs(K0 ** 6 - K1 ** 6) * d ** 4 / 90 * np.abs(phi).max() * 0.8


SEED = 20


@pytest.mark.parametrize("n,d", [(33, 1.0), (33, np.deg2rad(5.0) / 33), (64, np.deg2rad(5.0) / 64)])
def test_bound_admits_f64_intermediates_and_rejects_f32_ones(n, d):
    """The device order of operations in numpy.  With f64 intermediates every output stays inside the bound (measured
    for this seed: at most 0.99 of it, the f32 rounding of the output itself).  With f32 intermediates on
    phi = 1 + 1e-3 noise the outputs built from D2 leave it by 7e4 ... 1e7 times: 30 f[i] alone rounds at 2^-24 of 30
    while the result is a few 1e-2.  The alphas and gamma2 of that map cannot tell the two apart -- differences of
    neighbours of 1 are exact in f32 and so are their small-integer combinations (f32 ratios 0.66 ... 2.7) -- so they
    are told apart on white noise, where every output leaves the bound (14 ... 4e4 times)."""
    one = dn.noise_on_one(n, SEED)
    white = np.random.default_rng(SEED).standard_normal((n, n)).astype(np.float32)
    for phi, broken, factor in ((one, ("kappa", "gamma1", "gamma"), 1e4), (white, dn.FD_NAMES, 10)):
        ref = dn.fd_maps(phi, d)
        phi_max = float(np.abs(phi).max())
        e64, e32 = dn.fd_emulate(phi, d, np.float64), dn.fd_emulate(phi, d, np.float32)
        for k in dn.FD_NAMES:
            ok, worst = dn.fd_within_bound(k, e64[k], ref[k], phi_max, d)
            assert ok, (k, worst)
        for k in broken:
            ok, worst = dn.fd_within_bound(k, e32[k], ref[k], phi_max, d)
            assert not ok and worst > factor, (k, worst)


def test_emulation_is_exact_on_the_polynomials():
    """Every intermediate of the device order is an integer (or a dyadic fraction) on these maps, so kappa and gamma1
    come out without any rounding: what the GPU test asks of the kernel bit for bit."""
    n = 9
    i, j = grid(n)
    for f, d, want in (((i + j - 3) ** 3, 1.0, 6 * (i + j - 3)), ((i + j - 3) ** 2, 2.0, np.full((n, n), 0.5))):
        e = dn.fd_emulate(f.astype(np.float32), d, np.float64)
        assert np.array_equal(e["kappa"], want.astype(np.float32))
        assert np.array_equal(e["gamma1"], np.zeros((n, n), np.float32))


@pytest.mark.parametrize("n,band", [(5, 256), (23, 7), (40, 9), (41, 9)])
def test_banded_comparison_equals_the_plain_one(n, band):
    phi = dn.noise_on_one(n, n)
    ds = (1.0, 0.01)
    got = {d: dn.fd_emulate(phi, d, np.float64) for d in ds}
    worst = dn.fd_worst(phi, got, ds, band=band, workers=2)
    for d in ds:
        ref = dn.fd_maps(phi, d)
        for k in dn.FD_NAMES:
            # (the rescaled reference differs from the direct one by its own rounding, 2^-63 of it: 2^-38 of the error)
            plain = dn.fd_within_bound(k, got[d][k], ref[k], float(np.abs(phi).max()), d)[1]
            assert worst[d, k] == pytest.approx(plain, rel=1e-9), (d, k)
