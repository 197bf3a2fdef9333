"""Host side of the shear maps: the supported sizes, and the numpy restatement (tests/shear_np.py)
against analytic fields and against the complex-transform shortcut the contract rules out.  No GPU needed."""
import numpy as np
import pytest

import shear_np
import slicer_amd


@pytest.mark.parametrize("n,ok", [(32, 1), (30, 1), (45, 1), (49, 1), (4000, 1), (16384, 1), (2, 1), (15625, 1),
                                  (37, 0), (44, 0), (0, 0), (1, 0), (16385, 0), (-4, 0), (2 * 16384, 0)])
def test_supported_sizes(n, ok):
    assert slicer_amd.lensing._L.slicer_shear_supported(n) == ok
    assert slicer_amd.shear_supported(n) == bool(ok)


def test_sweep_lists_are_the_supported_sizes():
    """The size lists of tests/test_gpu_shear.py: every size slicer_shear_supported accepts, none other."""
    import test_gpu_shear as t
    every = [n for n in range(0, 16400) if slicer_amd.shear_supported(n)]
    assert len(every) == 399 and every == [n for n in range(0, 16400) if shear_np.seven_smooth(n)]
    assert t.SWEEP == [n for n in every if n <= 1200] and len(t.SWEEP) == 151
    assert t.SWEEP[:12] == [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15]
    assert t.SWEEP_SPLIT == [n for n in every if n <= 200]
    assert [n for n in every if n % 2 and n > 8192] == [8505, 8575, 9261, 9375, 10125, 10935, 11025, 11907, 12005,
                                                        13125, 14175, 15309, 15435, 15625]


@pytest.mark.parametrize("n,a,b", [(16, 3, 5), (45, -7, 11), (30, 4, 0), (45, 16, 0)])
def test_device_cosine_cases_agree_with_the_restatement(n, a, b):
    """cosine_case of tests/test_gpu_shear.py (the hand-made answers the device is held to) against shear_np."""
    import test_gpu_shear as t
    kappa, exact = t.cosine_case(n, a, b)
    out = shear_np.shear(kappa, 4.0)
    assert np.allclose(out["spectrum"], exact["spectrum"], atol=1e-9 * n * n)
    for k in ("phi", "gamma1", "gamma2"):
        assert np.allclose(out[k], exact[k], atol=1e-10 * np.abs(exact[k]).max() + 1e-13), k


@pytest.mark.parametrize("n,a,b", [(16, 1, 2), (16, 3, -1), (30, 2, 5), (45, 4, 7), (16, 8, 3), (16, 5, 8)])
def test_restatement_on_analytic_fields(n, a, b):
    """phi = A cos(2 pi (a i0 + b i1) / n): kappa = 1/2 lap phi, gamma1 = 1/2 (phi_00 - phi_11), gamma2 = phi_01, taken
    by hand; the restatement must return them from kappa (and phi itself when phi has no mean)."""
    angle, A = 4.0, 0.7
    theta = np.deg2rad(angle)
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    arg = 2 * np.pi * (a * i0 + b * i1) / n
    # wavenumbers of the mode as the restatement sees them: fftfreq along axis 0 (n/2 is -n/2), |b| along axis 1
    f0 = ((a + n // 2) % n) - n // 2 if n % 2 == 0 else ((a + (n - 1) // 2) % n) - (n - 1) // 2
    f1 = ((b + n // 2) % n) - n // 2 if n % 2 == 0 else ((b + (n - 1) // 2) % n) - (n - 1) // 2
    k0, k1 = 2 * np.pi * f0 / theta, 2 * np.pi * f1 / theta
    phi = A * np.cos(arg)
    kappa = -0.5 * (k0 ** 2 + k1 ** 2) * phi
    g1 = -0.5 * (k0 ** 2 - k1 ** 2) * phi
    g2 = -k0 * k1 * phi
    out = shear_np.shear(kappa, angle)
    scale = np.abs(phi).max()
    nyq = n % 2 == 0 and (f0 == -n // 2 or abs(f1) == n // 2)
    if not nyq:
        assert np.allclose(out["phi"], phi, atol=1e-10 * scale)
        assert np.allclose(out["gamma1"], g1, atol=1e-10 * np.abs(kappa).max())
        assert np.allclose(out["gamma2"], g2, atol=1e-10 * np.abs(kappa).max())
    else:
        # a Nyquist mode is real on the grid: cos survives, the 2 K0 K1 (odd) part of gamma2 does not where K1 = n/2
        assert np.allclose(out["gamma1"], g1, atol=1e-10 * np.abs(kappa).max())
        if abs(f1) == n // 2 and f1 != 0:
            assert np.allclose(out["gamma2"], 0.0, atol=1e-10 * np.abs(kappa).max())
        else:
            assert np.allclose(out["gamma2"], g2, atol=1e-10 * np.abs(kappa).max())
    assert np.allclose(out["gamma"], np.hypot(out["gamma1"], out["gamma2"]))


def test_axes_are_not_interchangeable():
    rng = np.random.default_rng(3)
    kappa = rng.standard_normal((16, 16))
    a, b = shear_np.shear(kappa, 2.0), shear_np.shear(kappa.T.copy(), 2.0)
    # swapping K0 and K1 flips the sign of gamma1 (up to Nyquist terms) and changes which Nyquist terms gamma2 keeps
    assert np.corrcoef(b["gamma1"].T.ravel(), a["gamma1"].ravel())[0, 1] < -0.5
    assert not np.allclose(b["gamma2"].T, a["gamma2"], atol=1e-3 * np.abs(a["gamma2"]).max())


def test_white_noise_differs_from_the_complex_shortcut():
    """16 x 16 white noise: the one-transform shortcut misses gamma2 by ~17 % of its max and leaks ~38 % into gamma1's
    real part; the restatement keeps irfft2's Hermitian projection."""
    rng = np.random.default_rng(16)
    kappa = rng.standard_normal((16, 16))
    ref = shear_np.shear(kappa, 5.0)
    s1, s2 = shear_np.shortcut_gamma(kappa, 5.0)
    d1 = np.abs(s1 - ref["gamma1"]).max() / np.abs(ref["gamma1"]).max()
    d2 = np.abs(s2 - ref["gamma2"]).max() / np.abs(ref["gamma2"]).max()
    assert d1 > 0.05 and d2 > 0.05, (d1, d2)
    # on a map without Nyquist content the two agree
    k = np.fft.rfft2(kappa)
    k[8, :] = 0
    k[:, 8] = 0
    smooth = np.fft.irfft2(k, s=(16, 16))
    ref = shear_np.shear(smooth, 5.0)
    s1, s2 = shear_np.shortcut_gamma(smooth, 5.0)
    assert np.allclose(s1, ref["gamma1"], atol=1e-12) and np.allclose(s2, ref["gamma2"], atol=1e-12)
