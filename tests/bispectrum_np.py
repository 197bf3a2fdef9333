"""f64 numpy restatement of the binned bispectrum contract, written from its formulas.

Bins are those of tests/power_np.py (edges in units of l_f, e2[b] <= m2 < e2[b + 1] on the integer m2, the last bin
closed) minus the mode m2 = 0.  Per bin F_b = irfft2(khat mask_b) and I_b = irfft2(mask_b), both f64; per triple
i <= j <= k: S = sum F_i F_j F_k, T = n^4 sum I_i I_j I_k, B = theta^4 / n^6 (n^4 S) / T, NaN where T < 0.5.
brute_force is the plain double loop over the full plane that both sums stand for."""
import numpy as np

import power_np


def all_triples(B):
    return np.array([(i, j, k) for i in range(B) for j in range(i, B) for k in range(j, B)], np.int32).reshape(-1, 3)


def equilateral_triples(B):
    return np.array([(b, b, b) for b in range(B)], np.int32).reshape(-1, 3)


def masks(n, edges):
    """bool [B][n][n // 2 + 1]: the half-plane modes of every bin."""
    edges = np.asarray(edges, np.float64)
    m2 = power_np.m2_rows(n, 0, n)
    idx = power_np.bin_index(m2, edges)
    idx[m2 == 0] = -1
    return np.stack([idx == b for b in range(edges.size - 1)])


def full_plane_counts(n, edges):
    """N_b: the modes of the full n x n plane in every bin."""
    return np.bincount(full_plane_bins(n, edges)[full_plane_bins(n, edges) >= 0], minlength=len(edges) - 1).astype(np.int64)


def full_plane_bins(n, edges):
    """int [n][n]: the bin of every mode of the full plane, -1 for none."""
    j = np.fft.fftfreq(n, 1.0 / n).round().astype(np.int64)
    m2 = j[:, None] ** 2 + j[None, :] ** 2
    idx = power_np.bin_index(m2, np.asarray(edges, np.float64))
    idx[m2 == 0] = -1
    return idx


def band_maps(spectrum, n, edges):
    """F [B][n][n] of a half-plane spectrum."""
    return np.stack([np.fft.irfft2(spectrum * m, s=(n, n)) for m in masks(n, edges)])


def indicator_maps(n, edges):
    """I [B][n][n]."""
    return np.stack([np.fft.irfft2(m.astype(np.complex128), s=(n, n)) for m in masks(n, edges)])


def triple_sums(F, triples):
    """sum_x (F_i F_j) F_k of every triple (numpy's pairwise sums)."""
    return np.array([np.sum((F[i] * F[j]) * F[k]) for i, j, k in np.asarray(triples).reshape(-1, 3)], np.float64)


def triangles(n, edges, triples):
    """T as the restatement has it (f64, close to an integer)."""
    return float(n) ** 4 * triple_sums(indicator_maps(n, edges), triples)


def bispectrum_of_spectrum(spectrum, n, angle_deg, edges, triples):
    """dict: b, triangles, sums, F (the band maps) from a half-plane spectrum."""
    theta = angle_deg * np.pi / 180.0
    F = band_maps(spectrum, n, edges)
    S = triple_sums(F, triples)
    T = triangles(n, edges, triples)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = np.where(T < 0.5, np.nan, theta ** 4 / float(n) ** 6 * (float(n) ** 4 * S) / T)
    return {"b": b, "triangles": T, "sums": S, "F": F}


def bispectrum(kappa, angle_deg, edges, triples):
    """The restatement from the map itself: f64 rfft2, then bispectrum_of_spectrum."""
    kappa = np.asarray(kappa, np.float64)
    return bispectrum_of_spectrum(np.fft.rfft2(kappa), kappa.shape[0], angle_deg, edges, triples)


def brute_force(kappa, edges, triples):
    """(n^4 S, T) of every triple by the double loop over the full plane, npix <= 16: T counts the ordered triples
    (l1 in i, l2 in j, l3 in k) with l1 + l2 + l3 = 0 modulo n on both axes, n^4 S sums khat(l1) khat(l2) khat(l3)
    over them."""
    kappa = np.asarray(kappa, np.float64)
    n = kappa.shape[0]
    assert n <= 16
    B = len(edges) - 1
    khat = np.fft.fft2(kappa)
    bins = full_plane_bins(n, edges)
    S = np.zeros((B, B, B), np.complex128)
    T = np.zeros((B, B, B), np.int64)
    for a0 in range(n):
        for a1 in range(n):
            bi = bins[a0, a1]
            if bi < 0:
                continue
            for b0 in range(n):
                for b1 in range(n):
                    bj = bins[b0, b1]
                    c0, c1 = (-a0 - b0) % n, (-a1 - b1) % n
                    bk = bins[c0, c1]
                    if bj < 0 or bk < 0:
                        continue
                    T[bi, bj, bk] += 1
                    S[bi, bj, bk] += khat[a0, a1] * khat[b0, b1] * khat[c0, c1]
    t = np.asarray(triples).reshape(-1, 3)
    assert np.abs(S.imag).max() <= 1e-9 * max(np.abs(S.real).max(), 1e-300)
    return S.real[t[:, 0], t[:, 1], t[:, 2]], T[t[:, 0], t[:, 1], t[:, 2]]
