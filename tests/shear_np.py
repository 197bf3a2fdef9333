"""f64 numpy restatement of the shear / lensing-potential contract, written from its formulas.

kappa is n x n, axis 0 the slow axis (K0, full spectrum), axis 1 the contiguous one (K1, half spectrum); the side of the
map is angle_deg degrees.  Every quotient by k^2 is 0 at k = 0."""
import numpy as np


def wavenumbers(n, angle_deg):
    d = np.deg2rad(angle_deg) / n
    k0 = 2 * np.pi * np.fft.fftfreq(n, d)[:, None]
    k1 = 2 * np.pi * np.fft.rfftfreq(n, d)[None, :]
    return k0, k1


def _over_k2(num, k2):
    out = np.zeros(np.broadcast(num, k2).shape)
    nz = np.broadcast_to(k2 != 0, out.shape)
    out[nz] = np.broadcast_to(num, out.shape)[nz] / np.broadcast_to(k2, out.shape)[nz]
    return out


def filters(n, angle_deg):
    """phi, gamma1 and gamma2 filters on the [n, n // 2 + 1] half spectrum."""
    k0, k1 = wavenumbers(n, angle_deg)
    k2 = k0 ** 2 + k1 ** 2
    return _over_k2(-2.0, k2), _over_k2(k0 ** 2 - k1 ** 2, k2), _over_k2(2 * k0 * k1, k2)


def shear(kappa, angle_deg):
    """dict: spectrum (rfft2 of kappa in f64), phi, gamma1, gamma2, gamma (f64, not rounded)."""
    kappa = np.asarray(kappa)
    n = kappa.shape[0]
    assert kappa.shape == (n, n)
    khat = np.fft.rfft2(kappa.astype(np.float64))
    fphi, fg1, fg2 = filters(n, angle_deg)
    out = {"spectrum": khat}
    for name, f in (("phi", fphi), ("gamma1", fg1), ("gamma2", fg2)):
        out[name] = np.fft.irfft2(khat * f, s=(n, n))
    out["gamma"] = np.sqrt(out["gamma1"] ** 2 + out["gamma2"] ** 2)
    return out


def shortcut_gamma(kappa, angle_deg):
    """The tempting shortcut the contract rules out: one full complex inverse of khat (K0^2 - K1^2 + 2i K0 K1) / k^2
    on the full spectrum, read as gamma1 + i gamma2."""
    n = kappa.shape[0]
    d = np.deg2rad(angle_deg) / n
    k0 = 2 * np.pi * np.fft.fftfreq(n, d)[:, None]
    k1 = 2 * np.pi * np.fft.fftfreq(n, d)[None, :]
    k2 = k0 ** 2 + k1 ** 2
    f = np.zeros((n, n), np.complex128)
    nz = k2 != 0
    f[nz] = ((k0 ** 2 - k1 ** 2 + 2j * k0 * k1) / np.where(nz, k2, 1.0))[nz]
    z = np.fft.ifft2(np.fft.fft2(np.asarray(kappa, np.float64)) * f)
    return z.real, z.imag


def seven_smooth(n):
    """The sizes the device transforms take: 2 <= n <= 16384 with no prime factor above 7."""
    if not 2 <= n <= 16384:
        return False
    for p in (2, 3, 5, 7):
        while n % p == 0:
            n //= p
    return n == 1


def within_bound(got, ref):
    """The f32 output bound: |got - ref| <= 2^-23 |ref| + 1e-9 max|ref|; returns (ok, worst ratio to the bound)."""
    got = np.asarray(got, np.float64)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-9 * np.abs(ref).max()
    ratio = np.abs(got - ref) / np.maximum(bound, np.finfo(np.float64).tiny)
    return bool((ratio <= 1.0).all()), float(ratio.max())


def clustered(n, seed, shape=0.3):
    """A clustered, kappa-like map: Gamma(shape) deviates, box-smoothed over 2 x 2 pixels, mean 0, f32."""
    rng = np.random.default_rng(seed)
    g = rng.gamma(shape, 1.0, (n, n))
    g = g + np.roll(g, 1, 0) + np.roll(g, 1, 1) + np.roll(np.roll(g, 1, 0), 1, 1)
    return (g - g.mean()).astype(np.float32) * np.float32(0.01)
