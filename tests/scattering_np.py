"""numpy restatement of the wavelet scattering coefficients of include/slicer_amd.h.

filter_bank follows the header's filter definition operation by operation in f64, so that it differs from
slicer_scattering_filter by the exponential alone.  coefficients takes the DIRECT route: the complex ifft2 of the full
plane, then the modulus; the library has no complex transform and goes through the Hermitian split, which
modulus_split restates, so the two are independent of one another.  modulus_dft is the long-double reference: the same
filters, every transform a direct O(n^4) DFT in np.longdouble."""
import math

import numpy as np

TWO_PI = 2.0 * math.pi
EPS = 2.0 ** -52


def signed(n):
    """The signed mode index of 0 .. n-1: a for a < (n + 1) // 2, else a - n (so that n/2 maps to -n/2)."""
    a = np.arange(n)
    return np.where(a < (n + 1) // 2, a, a - n).astype(np.float64)


def filter_constants(J, L, j, l):
    """sigma^2 / 2, xi, s^2, cos theta, sin theta of filter (j, l)."""
    sigma = 0.8 * 2.0 ** j
    xi = (3.0 * math.pi / 4.0) * 2.0 ** -j
    s = 4.0 / L
    theta = math.pi * l / L
    return sigma * sigma / 2.0, xi, s * s, math.cos(theta), math.sin(theta)


def alias_sums(w1, w2, c):
    """(A^, B^) at the angular frequencies w1 (axis 0), w2 (axis 1): the nine aliases, m1 outer, m2 inner, from -1 up."""
    h, xi, s2, ct, st = c
    w1, w2 = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
    A = np.zeros(np.broadcast(w1, w2).shape, np.float64)
    B = np.zeros_like(A)
    for m1 in (-1, 0, 1):
        for m2 in (-1, 0, 1):
            v1, v2 = w1 + TWO_PI * m1, w2 + TWO_PI * m2
            p = v1 * ct + v2 * st
            q = -v1 * st + v2 * ct
            d = p - xi
            A = A + np.exp(-h * (d * d + q * q / s2))
            B = B + np.exp(-h * (p * p + q * q / s2))
    return A, B


def filter_parts(n, J, L, j, l):
    """(A^, beta B^) over the full [n][n] mode plane: psi^ is their difference away from [0, 0]."""
    c = filter_constants(J, L, j, l)
    A0, B0 = alias_sums(0.0, 0.0, c)
    beta = float(A0) / float(B0)
    w = TWO_PI * signed(n) / n
    A, B = alias_sums(w[:, None], w[None, :], c)
    return A, beta * B


def filter_bank(n, J, L, j, l):
    """psi^_{jl}[a][b] over the full mode plane, f64, [0, 0] exactly 0."""
    A, bB = filter_parts(n, J, L, j, l)
    psi = A - bB
    psi[0, 0] = 0.0
    return psi


def bank(n, J, L):
    return [[filter_bank(n, J, L, j, l) for l in range(L)] for j in range(J)]


def modulus(f, psi):
    """|ifft2(fft2(f) psi^)| of a real f64 field: the direct complex route."""
    return np.abs(np.fft.ifft2(np.fft.fft2(f) * psi))


def modulus_split(f, psi):
    """The library's route: E and O over the mode indices, two real inverses, u = sqrt(x x + y y)."""
    n = f.shape[0]
    neg = (-np.arange(n)) % n
    flip = psi[np.ix_(neg, neg)]
    E, O = (psi + flip) / 2.0, (psi - flip) / 2.0
    H = n // 2 + 1
    fh = np.fft.rfft2(f)
    x = np.fft.irfft2(fh * E[:, :H], s=(n, n))
    y = np.fft.irfft2(-1j * fh * O[:, :H], s=(n, n))
    return np.sqrt(x * x + y * y)


def coefficients(kappa, J, L, route=modulus, between=None, banks=None):
    """{"s0": [2], "s1": [J][L], "p1": [J][L], "s2": [J][L][J][L] (NaN for j2 <= j1)} of an f32 or f64 n^2 map.
    between: applied to u1 before the second order (the f32 sharpness check rounds there)."""
    k = np.asarray(kappa, np.float64)
    n = k.shape[0]
    psi = banks if banks is not None else bank(n, J, L)
    s1, p1 = np.zeros((J, L)), np.zeros((J, L))
    s2 = np.full((J, L, J, L), np.nan)
    for j1 in range(J):
        for l1 in range(L):
            u = route(k, psi[j1][l1])
            s1[j1, l1] = u.mean()
            p1[j1, l1] = (u * u).mean()
            if between is not None:
                u = between(u)
            for j2 in range(j1 + 1, J):
                for l2 in range(L):
                    s2[j1, l1, j2, l2] = route(u, psi[j2][l2]).mean()
    return {"s0": np.array([k.mean(), (k * k).mean()]), "s1": s1, "p1": p1, "s2": s2}


def dft_matrix(n, sign):
    """exp(sign 2 pi i a x / n) in long double, the angle reduced exactly through (a x) mod n."""
    ax = (np.outer(np.arange(n), np.arange(n)) % n).astype(np.longdouble)
    t = 2.0 * np.arccos(np.longdouble(-1.0)) * ax / np.longdouble(n)
    return np.cos(t) + sign * 1j * np.sin(t)


def modulus_dft(f, psi, mats):
    """modulus() with both transforms as direct DFTs in long double.  mats = (dft_matrix(n, -1), dft_matrix(n, +1))."""
    F, G = mats
    n = f.shape[0]
    fl = np.asarray(f, np.longdouble)
    hat = F @ fl @ F
    z = (G @ (hat * np.asarray(psi, np.longdouble)) @ G) / (np.longdouble(n) * np.longdouble(n))
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def coefficients_dft(kappa, J, L):
    """coefficients() in long double throughout (the filters are the f64 ones)."""
    k = np.asarray(kappa, np.float64)
    n = k.shape[0]
    mats = (dft_matrix(n, -1), dft_matrix(n, +1))
    out = coefficients(k, J, L, route=lambda f, p: modulus_dft(f, p, mats))
    return out


def unit(kappa, per_pixel=False):
    """U = 2^-52 log2(n) sqrt(mean kappa^2); per pixel on max |kappa| instead."""
    k = np.asarray(kappa, np.float64)
    scale = float(np.abs(k).max()) if per_pixel else math.sqrt(float((k * k).mean()))
    return EPS * math.log2(k.shape[0]) * scale


REF_U = 0.14     # what the numpy route itself shows against the long-double DFT (test_scattering_host.py re-measures it)
DEVICE_U = 16 * REF_U


def device_bound(value, u):
    """The device's bound against this restatement: 16 x 0.14 U for the other radix order of its transform, and 64 ulp
    of the value for exp and its argument."""
    return DEVICE_U * u + 64 * EPS * np.abs(value)


def reduce_np(s1, s2):
    """Orientation averages: s1(j) and s2(j1, j2, (l2 - l1) mod L), by plain loops."""
    J, L = s1.shape
    r1 = np.array([sum(s1[j, l] for l in range(L)) / L for j in range(J)])
    r2 = np.full((J, J, L), np.nan)
    for j1 in range(J):
        for j2 in range(j1 + 1, J):
            for d in range(L):
                r2[j1, j2, d] = sum(s2[j1, l1, j2, (l1 + d) % L] for l1 in range(L)) / L
    return r1, r2


def white(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)


def lognormal(n, seed):
    """A smoothed Gaussian field, exponentiated and shifted to zero mean: skewed like a convergence map."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, n))
    k = np.fft.fftfreq(n)
    k2 = k[:, None] ** 2 + k[None, :] ** 2
    g = np.fft.ifft2(np.fft.fft2(g) * np.exp(-k2 * 40.0)).real
    g /= g.std()
    x = np.exp(0.8 * g)
    return (0.02 * (x - x.mean())).astype(np.float32)
