"""f64 numpy restatement of the binned power-spectrum contract, written from its formulas.

Maps are n x n, axis 0 the slow axis (j0 = signed fftfreq index), axis 1 the contiguous one (j1 = rfft index).  Every
coefficient of the [n][n // 2 + 1] half plane is one mode of integer radius^2 m2 = j0^2 + j1^2; edges are radii in
units of l_f = 2 pi / theta, and a mode is in bin b iff e2[b] <= m2 < e2[b + 1], e2 = edges * edges in f64, the last
bin closed on the right.  C_st,b = theta^2 / n^4 / N_b * sum over the bin of Re(khat_s conj khat_t)."""
import numpy as np

CHUNK = 16  # rows per bincount: short sums, so the binned sums stay accurate to a few ulp at 16384^2


def ell_f(angle_deg):
    return 2.0 * np.pi / (angle_deg * np.pi / 180.0)


def default_edges(n):
    return np.arange(n, dtype=np.float64)


def m2_rows(n, i0, i1):
    """Integer radius^2 of the half-plane modes of rows i0 .. i1 - 1."""
    j0 = np.fft.fftfreq(n, 1.0 / n).round().astype(np.int64)[i0:i1, None]
    j1 = np.arange(n // 2 + 1, dtype=np.int64)[None, :]
    return j0 * j0 + j1 * j1


def bin_index(m2, edges):
    """Bin of every mode (searchsorted on the edge squares, the last bin closed); -1: in no bin."""
    e2 = np.asarray(edges, np.float64) ** 2
    B = e2.size - 1
    x = m2.astype(np.float64)  # exact: m2 < 2^53
    idx = np.searchsorted(e2, x, side="right") - 1
    idx[x == e2[-1]] = B - 1
    idx[(idx < 0) | (idx >= B)] = -1
    return idx


def binned_sums(n, edges, weights=()):
    """counts [B] and, for every [n][n // 2 + 1] array in weights, its sum per bin [B] (row chunks of CHUNK)."""
    B = len(edges) - 1
    counts = np.zeros(B, np.int64)
    sums = [np.zeros(B) for _ in weights]
    for i0 in range(0, n, CHUNK):
        i1 = min(n, i0 + CHUNK)
        idx = bin_index(m2_rows(n, i0, i1), edges).ravel()
        keep = idx >= 0
        counts += np.bincount(idx[keep], minlength=B)
        for k, w in enumerate(weights):
            sums[k] += np.bincount(idx[keep], weights=np.asarray(w[i0:i1]).ravel()[keep], minlength=B)
    return counts, sums


def bins(n, edges=None):
    """counts and mean radius (units of l_f) per bin; the radius of a mode depends on |j0|, so the sums run over rows
    of one sign and weight the rows that exist twice."""
    edges = default_edges(n) if edges is None else np.asarray(edges, np.float64)
    B = edges.size - 1
    counts = np.zeros(B, np.int64)
    rsum = np.zeros(B)
    for a0 in range(0, n // 2 + 1, CHUNK):
        a = np.arange(a0, min(n // 2 + 1, a0 + CHUNK), dtype=np.int64)
        mult = (a <= (n - 1) // 2).astype(np.int64) + ((a >= 1) & (a <= n // 2)).astype(np.int64)
        m2 = a[:, None] ** 2 + np.arange(n // 2 + 1, dtype=np.int64)[None, :] ** 2
        idx = bin_index(m2, edges)
        w = np.broadcast_to(mult[:, None], m2.shape)
        keep = (idx >= 0) & (w > 0)
        counts += np.bincount(idx[keep], weights=w[keep], minlength=B).round().astype(np.int64)
        rsum += np.bincount(idx[keep], weights=(w * np.sqrt(m2.astype(np.float64)))[keep], minlength=B)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(counts > 0, rsum / np.maximum(counts, 1), np.nan)
    return counts, mean


def pairs(S, cross):
    return [(s, t) for s in range(S) for t in range(s, S)] if cross else [(s, s) for s in range(S)]


def power_of_spectra(spectra, angle_deg, edges=None, cross=False):
    """dict: counts, cl ([S][S][B] symmetric with cross, else [S][B]) and scale ([same]: theta^2 / n^4 times the bin
    mean of |khat_s| |khat_t|, the size of the terms of C_st,b) from the half-plane spectra."""
    S = len(spectra)
    n = spectra[0].shape[0]
    edges = default_edges(n) if edges is None else np.asarray(edges, np.float64)
    theta = angle_deg * np.pi / 180.0
    norm = theta * theta / float(n) ** 4
    pl = pairs(S, cross)
    w = []
    for s, t in pl:
        a, b = spectra[s], spectra[t]
        w.append(a.real * b.real + a.imag * b.imag)
        w.append(np.abs(a) * np.abs(b))
    counts, sums = binned_sums(n, edges, w)
    B = edges.size - 1
    shape = (S, S, B) if cross else (S, B)
    cl, scale = np.full(shape, np.nan), np.full(shape, np.nan)
    nz = counts > 0
    for k, (s, t) in enumerate(pl):
        c = np.full(B, np.nan)
        m = np.full(B, np.nan)
        c[nz] = norm * (sums[2 * k][nz] / counts[nz])
        m[nz] = norm * (sums[2 * k + 1][nz] / counts[nz])
        if cross:
            cl[s, t] = cl[t, s] = c
            scale[s, t] = scale[t, s] = m
        else:
            cl[s], scale[s] = c, m
    return {"counts": counts, "cl": cl, "scale": scale}


def power(maps, angle_deg, edges=None, cross=False):
    """The restatement from the maps themselves: f64 rfft2, then power_of_spectra."""
    return power_of_spectra([np.fft.rfft2(np.asarray(m, np.float64)) for m in maps], angle_deg, edges, cross)
