"""f64 numpy restatement of the masked pseudo-C_l contract, written from its formulas; the
notation and the bins are those of power_np (row N7).

H_b: the half-plane coefficients of bin b (each one mode), N_b their number; F_b: the full-plane modes whose m2 lies in
bin b, m2 = 0 included.  With what = fft2(w) unnormalised,
  M[b][b'] = 1 / (N_b n^4) * sum over k in H_b, k' in F_b' of |what(k - k')|^2
and the decoupled bandpowers are M_act^-1 applied to the coupled ones on the bins with N_b > 0 (NaN in the others)."""
import numpy as np

import power_np


def taper(n, width_pix):
    """f [n]: x_i = min(i, n-1-i) + 0.5, t = x_i / width_pix, f = 1 for t >= 1, else t - sin(2 pi t) / (2 pi)."""
    i = np.arange(n)
    t = (np.minimum(i, n - 1 - i) + 0.5) / float(width_pix)
    return np.where(t >= 1.0, 1.0, t - np.sin(2 * np.pi * t) / (2 * np.pi))


def mask(n, width_pix=0.0, user=None):
    """w as the device rounds it: float32(f[i0] f[i1]) (the product in f64), times the f32 user mask in f32."""
    if width_pix > 0:
        f = taper(n, width_pix)
        w = (f[:, None] * f[None, :]).astype(np.float32)
        return w if user is None else w * np.asarray(user, np.float32)
    return np.array(user, np.float32)


def full_plane_bins(n, edges):
    """Bin of every mode of the full [n][n] plane, -1: in no bin."""
    j = np.fft.fftfreq(n, 1.0 / n).round().astype(np.int64)
    return power_np.bin_index(j[:, None] ** 2 + j[None, :] ** 2, edges)


def coupling_fft(w, edges):
    """M by the autocorrelation route: A = irfft2(|rfft2 w|^2), G_b' = irfft2 of the indicator of F_b' (ifft2 of the
    full-plane indicator, which is real), Q = Re rfft2(A G) / n^2, M[b][b'] = mean of Q over H_b.  Rows and columns of
    empty bins are 0."""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    A = np.fft.irfft2(np.abs(np.fft.rfft2(w)) ** 2, s=(n, n))
    full = full_plane_bins(n, edges)
    counts, _ = power_np.binned_sums(n, edges)
    M = np.zeros((B, B))
    for bp in range(B):
        if counts[bp] == 0:
            continue
        G = np.fft.ifft2((full == bp).astype(np.float64)).real
        Q = np.fft.rfft2(A * G).real / float(n * n)
        _, (s,) = power_np.binned_sums(n, edges, [Q])
        nz = counts > 0
        M[nz, bp] = s[nz] / counts[nz]
    return M


def coupling_brute(w, edges):
    """M by the double sum itself, O(n^4): small n only."""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    P = np.abs(np.fft.fft2(w)) ** 2
    full = full_plane_bins(n, edges)
    half = power_np.bin_index(power_np.m2_rows(n, 0, n), edges)
    counts = np.bincount(half[half >= 0], minlength=B)
    M = np.zeros((B, B))
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for k0 in range(n):
        for k1 in range(n // 2 + 1):
            b = half[k0, k1]
            if b < 0:
                continue
            d = P[(k0 - i0) % n, (k1 - i1) % n]  # |what(k - k')|^2 for every k' = (i0, i1)
            keep = full >= 0
            M[b] += np.bincount(full[keep], weights=d[keep], minlength=B)
    nz = counts > 0
    M[nz] /= counts[nz, None] * float(n) ** 4
    M[:, ~nz] = 0.0
    return M


def coupled(maps, w, angle_deg, edges, cross=False):
    """power_np.power of the f32 products w * kappa."""
    w = np.asarray(w, np.float32)
    return power_np.power([w * np.asarray(m, np.float32) for m in maps], angle_deg, edges, cross)


def decouple(M, cl_coupled, counts):
    """M_act^-1 on the last axis of cl_coupled over the bins with counts > 0; NaN in the others."""
    act = np.flatnonzero(np.asarray(counts) > 0)
    c = np.asarray(cl_coupled, np.float64)
    out = np.full(c.shape, np.nan)
    Ma = np.asarray(M)[np.ix_(act, act)]
    flat = c.reshape(-1, c.shape[-1])
    o = out.reshape(-1, c.shape[-1])
    for r in range(flat.shape[0]):
        o[r, act] = np.linalg.solve(Ma, flat[r, act])
    return out


def pcl(maps, w, angle_deg, edges, cross=False):
    """dict: counts, coupled, cl, M -- the whole contract from the maps and the mask."""
    ref = coupled(maps, w, angle_deg, edges, cross)
    M = coupling_fft(w, edges)
    return {"counts": ref["counts"], "coupled": ref["cl"], "M": M, "cl": decouple(M, ref["cl"], ref["counts"])}
