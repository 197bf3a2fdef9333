"""numpy restatement of the deflection and finite-difference contract, written from its formulas.

Spectral deflection: np.fft.rfft2 / irfft2 in f64, in the notation of tests/shear_np.py.  Finite differences: the line
operators D1 and D2 in np.longdouble, applied along axis 0 (slow) and axis 1 (contiguous) of an n x n map, n >= 5."""
import numpy as np

import shear_np

FD_NAMES = ("alpha1", "alpha2", "kappa", "gamma1", "gamma2", "gamma")  # in the order of the SLICER_FD_* codes


def deflection(kappa, angle_deg):
    """alpha1 = irfft2(i K0 phihat), alpha2 = irfft2(i K1 phihat), phihat = -2 khat / k^2 (0 at k = 0); f64, radians."""
    kappa = np.asarray(kappa)
    n = kappa.shape[0]
    assert kappa.shape == (n, n)
    k0, k1 = shear_np.wavenumbers(n, angle_deg)
    phihat = np.fft.rfft2(kappa.astype(np.float64)) * shear_np.filters(n, angle_deg)[0]
    return np.fft.irfft2(1j * k0 * phihat, s=(n, n)), np.fft.irfft2(1j * k1 * phihat, s=(n, n))


def d1(f, d, axis):
    """(f[i-2] - 8 f[i-1] + 8 f[i+1] - f[i+2]) / (12 d) for 2 <= i <= n-3; (f[i+1] - f[i]) / d at i = 0, 1;
    (f[i] - f[i-1]) / d at i = n-2, n-1."""
    f = np.moveaxis(np.asarray(f, np.longdouble), axis, 0)
    d = np.longdouble(d)
    assert f.shape[0] >= 5
    out = np.empty_like(f)
    out[2:-2] = (f[:-4] - 8 * f[1:-3] + 8 * f[3:-1] - f[4:]) / (12 * d)
    out[:2] = (f[1:3] - f[:2]) / d
    out[-2:] = (f[-2:] - f[-3:-1]) / d
    return np.moveaxis(out, 0, axis)


def d2(f, d, axis):
    """(-f[i-2] + 16 f[i-1] - 30 f[i] + 16 f[i+1] - f[i+2]) / (12 d^2) for 2 <= i <= n-3;
    (2 f[i] - 5 f[i+1] + 4 f[i+2] - f[i+3]) / d^2 at i = 0, 1; (2 f[i] - 5 f[i-1] + 4 f[i-2] - f[i-3]) / d^2 at
    i = n-2, n-1."""
    f = np.moveaxis(np.asarray(f, np.longdouble), axis, 0)
    d = np.longdouble(d)
    assert f.shape[0] >= 5
    out = np.empty_like(f)
    out[2:-2] = (-f[:-4] + 16 * f[1:-3] - 30 * f[2:-2] + 16 * f[3:-1] - f[4:]) / (12 * d * d)
    out[:2] = (2 * f[:2] - 5 * f[1:3] + 4 * f[2:4] - f[3:5]) / (d * d)
    out[-2:] = (2 * f[-2:] - 5 * f[-3:-1] + 4 * f[-4:-2] - f[-5:-3]) / (d * d)
    return np.moveaxis(out, 0, axis)


def fd_maps(phi, d):
    """dict of the six outputs (FD_NAMES) plus p12 and p21, in longdouble, not rounded."""
    phi = np.asarray(phi, np.longdouble)
    p11, p22 = d2(phi, d, 0), d2(phi, d, 1)
    a1, a2 = d1(phi, d, 0), d1(phi, d, 1)
    p12, p21 = d1(a1, d, 1), d1(a2, d, 0)
    g1, g2 = (p11 - p22) / 2, (p12 + p21) / 2
    return {"alpha1": a1, "alpha2": a2, "kappa": (p11 + p22) / 2, "gamma1": g1, "gamma2": g2,
            "gamma": np.sqrt(g1 * g1 + g2 * g2), "p12": p12, "p21": p21}


def rescale(maps, d_from, d_to):
    """fd_maps(phi, d_to) from fd_maps(phi, d_from): every output is homogeneous in the spacing (degree -1 for the
    alphas, -2 for the rest), so a second spacing costs no second pass of stencils."""
    r = np.longdouble(d_from) / np.longdouble(d_to)
    return {k: v * (r if k in ("alpha1", "alpha2") else r * r) for k, v in maps.items()}


# f64 roundings on the longest path of the device evaluation, counted from slicer_fd.hip (its header comment):
#   D1: the numerator (f[i-2] - f[i+2]) + 8 (f[i+1] - f[i-1]) 2, the denominator 12 d 1, the division 1
#   D2: the numerator (16 (f[i-1] + f[i+1]) - (f[i-2] + f[i+2])) - 30 f[i] 3, the denominator 12 (d d) 2, the division 1
#   kappa, gamma1: D2 and the sum or difference of p11 and p22 (halving is exact)
#   gamma2 = p12: a D1 numerator of D1 numerators 4, the two denominators and their product 3, the division 1
K_ALPHA, K_P, K_KAPPA, K_MIXED = 4, 6, 7, 8
W_ALPHA, W_P, W_MIXED = 2, 12, 4  # the largest absolute weight sums: 1 + 1;  2 + 5 + 4 + 1;  (1 + 1)^2
# |gamma| = sqrt(g1^2 + g2^2) is 1-Lipschitz in (g1, g2), so errors e1, e2 of the components move it by at most
# e1 + e2; its own evaluation rounds the two squares and their sum (relative 2 u of the radicand, 1 u of the root) and
# the root (1 u): 2 u |gamma| <= 2 u (|g1| + |g2|) <= 2 u (W_P + W_MIXED) max|phi| / d^2.
KW_GAMMA = K_KAPPA * W_P + K_MIXED * W_MIXED + 2 * (W_P + W_MIXED)
KW = {"alpha1": K_ALPHA * W_ALPHA, "alpha2": K_ALPHA * W_ALPHA, "kappa": K_KAPPA * W_P, "gamma1": K_KAPPA * W_P,
      "gamma2": K_MIXED * W_MIXED, "gamma": KW_GAMMA}


def fd_bound(name, ref, phi_max, d):
    """2^-24 |ref| (1 + 2^-20) + K 2^-53 W max|phi| / d^q: one f32 rounding plus the f64 roundings of the evaluation."""
    q = 1 if name in ("alpha1", "alpha2") else 2
    floor = KW[name] * 2.0 ** -53 * float(phi_max) / float(d) ** q
    return 2.0 ** -24 * np.abs(ref).astype(np.float64) * (1 + 2.0 ** -20) + floor


def fd_within_bound(name, got, ref, phi_max, d):
    """(ok, worst ratio to the bound)"""
    err = np.abs(np.asarray(got, np.longdouble) - ref).astype(np.float64)
    ratio = err / fd_bound(name, ref, phi_max, d)
    return bool((ratio <= 1.0).all()), float(ratio.max())


def fd_worst(phi, got, spacings, band=256, workers=16):
    """{(d, name): worst ratio of |got[d][name] - fd_maps(phi, d)[name]| to fd_bound} over the whole map.  The reference
    is taken in bands of rows with four rows of margin (no stencil reaches further; the one-sided rows of a band lie in
    its margin unless they are the map's own) on a few threads: numpy's long double is slow."""
    from concurrent.futures import ThreadPoolExecutor
    phi = np.asarray(phi, np.float32)
    n = phi.shape[0]
    phi_max = float(np.abs(phi).max())

    def one(r0):
        r1 = min(n, r0 + band)
        if n - r1 < 5:  # no sliver of a last band
            r1 = n
        lo, hi = max(0, r0 - 4), min(n, r1 + 4)
        unit = {k: v[r0 - lo:r1 - lo] for k, v in fd_maps(phi[lo:hi], 1.0).items() if k in FD_NAMES}
        out = {}
        for d in spacings:
            ref = rescale(unit, 1.0, d)
            for k in FD_NAMES:
                out[d, k] = fd_within_bound(k, got[d][k][r0:r1], ref[k], phi_max, d)[1]
        return r1, out

    starts, r = [], 0
    while r < n:
        starts.append(r)
        r = n if n - (r + band) < 5 else r + band
    with ThreadPoolExecutor(max_workers=workers) as ex:
        parts = [o for _, o in ex.map(one, starts)]
    return {key: max(p[key] for p in parts) for key in parts[0]}


def fd_emulate(phi, d, dtype):
    """The device's order of operations (slicer_fd.hip) with every intermediate held in `dtype`; outputs rounded to f32."""
    t = dtype
    f = np.asarray(phi, np.float32).astype(t)
    n = f.shape[0]
    d = t(d)
    den1, dd = t(12) * d, d * d
    den2 = t(12) * dd

    def num1(g, axis):
        g = np.moveaxis(g, axis, 0)
        out = np.empty_like(g)
        out[2:-2] = (g[:-4] - g[4:]) + t(8) * (g[3:-1] - g[1:-3])
        out[:2] = g[1:3] - g[:2]
        out[-2:] = g[-2:] - g[-3:-1]
        return np.moveaxis(out, 0, axis)

    def num2(g, axis):
        g = np.moveaxis(g, axis, 0)
        out = np.empty_like(g)
        out[2:-2] = (t(16) * (g[1:-3] + g[3:-1]) - (g[:-4] + g[4:])) - t(30) * g[2:-2]
        out[:2] = (t(2) * g[:2] - t(5) * g[1:3]) + (t(4) * g[2:4] - g[3:5])
        out[-2:] = (t(2) * g[-2:] - t(5) * g[-3:-1]) + (t(4) * g[-4:-2] - g[-5:-3])
        return np.moveaxis(out, 0, axis)

    edge = np.zeros(n, bool)
    edge[:2] = edge[-2:] = True
    e1 = np.where(edge, d, den1).astype(t)   # denominator of D1 per sample of a line
    e2 = np.where(edge, dd, den2).astype(t)
    a1, a2 = num1(f, 0) / e1[:, None], num1(f, 1) / e1[None, :]
    p11, p22 = num2(f, 0) / e2[:, None], num2(f, 1) / e2[None, :]
    g1 = t(0.5) * (p11 - p22)
    g2 = num1(num1(f, 0), 1) / (e1[:, None] * e1[None, :])
    out = {"alpha1": a1, "alpha2": a2, "kappa": t(0.5) * (p11 + p22), "gamma1": g1, "gamma2": g2,
           "gamma": np.sqrt(g1 * g1 + g2 * g2)}
    return {k: v.astype(np.float32) for k, v in out.items()}


def noise_on_one(n, seed):
    """phi = 1 + 1e-3 noise: the differences cancel three digits, which f32 intermediates do not survive."""
    rng = np.random.default_rng(seed)
    return (1.0 + 1e-3 * rng.standard_normal((n, n))).astype(np.float32)
