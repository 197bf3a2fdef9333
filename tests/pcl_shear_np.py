"""f64 numpy restatement of the E/B pseudo-C_l contract, written from its formulas; the
notation, the bins and the mask are those of power_np (row N7) and pcl_np (row N17).

For a mode (j0, j1) with m2 = j0^2 + j1^2 > 0: c2 = (j0^2 - j1^2) / m2, s2 = 2 j0 j1 / m2, c4 = c2 c2 - s2 s2,
s4 = 2 (c2 s2), one rounding per operation; (1, 0) at m2 = 0; on the Nyquist lines of an even n the sines are 0.
  Ehat = c2 g1 + s2 g2, Bhat = c2 g2 - s2 g1
  M_s[b][b'] = 1 / (N_b n^4) sum over k in H_b, k' in F_b' of |what(k - k')|^2 (C_s(k) C_s(k') + S_s(k) S_s(k'))
  X_s[b][b'] = the same with (C_s(k) S_s(k') - S_s(k) C_s(k'))
and the decoupling solves M_0 (kk), [[M_2, -X_2], [X_2, M_2]] (kE, kB) and the 4 x 4 block system of P = (M_0 + M_4) / 2,
R = (M_0 - M_4) / 2, T = X_4 / 2 (EE, EB, BE, BB) on the bins with N_b > 0."""
import numpy as np

import pcl_np
import power_np


def _phases(n, j0, j1, spin):
    j0, j1 = np.broadcast_arrays(j0.astype(np.float64), j1.astype(np.float64))
    a, b = j0 * j0, j1 * j1
    m2 = a + b
    safe = np.where(m2 == 0.0, 1.0, m2)
    c2 = (a - b) / safe
    s2 = (2.0 * j0 * j1) / safe
    if spin == 2:
        c, s = c2, s2
    else:
        assert spin == 4
        c = c2 * c2 - s2 * s2
        s = 2.0 * (c2 * s2)
    if n % 2 == 0:
        s = np.where((np.abs(j0) == n // 2) | (np.abs(j1) == n // 2), 0.0, s)
    return np.where(m2 == 0.0, 1.0, c), np.where(m2 == 0.0, 0.0, s)


def phases(n, spin):
    """(C_s, S_s) on the [n][n // 2 + 1] half plane."""
    j0 = np.fft.fftfreq(n, 1.0 / n).round()[:, None]
    return _phases(n, j0, np.arange(n // 2 + 1, dtype=np.float64)[None, :], spin)


def phases_full(n, spin):
    """(C_s, S_s) on the full [n][n] plane."""
    j = np.fft.fftfreq(n, 1.0 / n).round()
    return _phases(n, j[:, None], j[None, :], spin)


def rotate(g1, g2):
    """(Ehat, Bhat) of the half-plane spectra g1, g2: the products rounded, then the sums, on re and im separately."""
    c, s = phases(g1.shape[0], 2)
    e, b = np.empty(g1.shape, np.complex128), np.empty(g1.shape, np.complex128)
    e.real, e.imag = c * g1.real + s * g2.real, c * g1.imag + s * g2.imag  # (set part by part: the signs of zeros stay)
    b.real, b.imag = c * g2.real - s * g1.real, c * g2.imag - s * g1.imag
    return e, b


def coupling_fft(w, edges, spin):
    """(M_s, X_s) by the autocorrelation route: A = irfft2(|rfft2 w|^2); per b', G_c and G_s = ifft2 of C_s and S_s inside
    F_b', Q = Re rfft2(A G) / n^2, and the means over H_b of C_s Q_c + S_s Q_s and C_s Q_s - S_s Q_c."""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    A = np.fft.irfft2(np.abs(np.fft.rfft2(w)) ** 2, s=(n, n))
    full = pcl_np.full_plane_bins(n, edges)
    counts, _ = power_np.binned_sums(n, edges)
    C, S = phases(n, spin)
    Cf, Sf = phases_full(n, spin)
    M, X = np.zeros((B, B)), np.zeros((B, B))
    nz = counts > 0
    for bp in range(B):
        if counts[bp] == 0:
            continue
        ind = (full == bp).astype(np.float64)
        Qc = np.fft.rfft2(A * np.fft.ifft2(ind * Cf).real).real / float(n * n)
        Qs = np.fft.rfft2(A * np.fft.ifft2(ind * Sf).real).real / float(n * n)
        _, (m, x) = power_np.binned_sums(n, edges, [C * Qc + S * Qs, C * Qs - S * Qc])
        M[nz, bp] = m[nz] / counts[nz]
        X[nz, bp] = x[nz] / counts[nz]
    return M, X


def coupling_brute(w, edges, spin):
    """(M_s, X_s) by the double sums themselves, O(n^4): small n only."""
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    P = np.abs(np.fft.fft2(w)) ** 2
    full = pcl_np.full_plane_bins(n, edges)
    half = power_np.bin_index(power_np.m2_rows(n, 0, n), edges)
    counts = np.bincount(half[half >= 0], minlength=B)
    C, S = phases(n, spin)
    Cf, Sf = phases_full(n, spin)
    M, X = np.zeros((B, B)), np.zeros((B, B))
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = full >= 0
    for k0 in range(n):
        for k1 in range(n // 2 + 1):
            b = half[k0, k1]
            if b < 0:
                continue
            d = P[(k0 - i0) % n, (k1 - i1) % n]  # |what(k - k')|^2 for every k' = (i0, i1)
            c, s = C[k0, k1], S[k0, k1]
            M[b] += np.bincount(full[keep], weights=(d * (c * Cf + s * Sf))[keep], minlength=B)
            X[b] += np.bincount(full[keep], weights=(d * (c * Sf - s * Cf))[keep], minlength=B)
    nz = counts > 0
    for Y in (M, X):
        Y[nz] /= counts[nz, None] * float(n) ** 4
        Y[:, ~nz] = 0.0
    return M, X


def system2(M2, X2):
    """The (kE, kB) system."""
    return np.block([[M2, -X2], [X2, M2]])


def system4(M0, M4, X4):
    """The (EE, EB, BE, BB) system."""
    P, R, T = (M0 + M4) / 2.0, (M0 - M4) / 2.0, X4 / 2.0
    return np.block([[P, -T, -T, R], [T, P, -R, -T], [T, -R, P, -T], [R, T, T, P]])


def solve_blocks(system, rows, act):
    """system restricted to the active bins, applied to the rows [m][B] of coupled bandpowers; NaN in the other bins."""
    act = np.flatnonzero(act)
    m, B = len(rows), len(rows[0])
    idx = np.concatenate([k * B + act for k in range(m)])
    x = np.linalg.solve(system[np.ix_(idx, idx)], np.concatenate([np.asarray(r)[act] for r in rows]))
    out = np.full((m, B), np.nan)
    out[:, act] = x.reshape(m, act.size)
    return out


def matrices(w, edges, brute=False):
    """dict M0, M2, X2, M4, X4 of the mask."""
    route = coupling_brute if brute else coupling_fft
    M2, X2 = route(w, edges, 2)
    M4, X4 = route(w, edges, 4)
    M0 = pcl_np.coupling_brute(w, edges) if brute else pcl_np.coupling_fft(w, edges)
    return {"M0": M0, "M2": M2, "X2": X2, "M4": M4, "X4": X4}


def decouple(mats, coupled, counts, cross):
    """The named decoupled bandpowers from the named coupled ones (EE, EB, BE, BB[, kE, kB, Ek, Bk, kk]), each
    [F][F][B] (cross) or [F][B]."""
    act = np.asarray(counts) > 0
    s4 = system4(mats["M0"], mats["M4"], mats["X4"])
    s2 = system2(mats["M2"], mats["X2"])
    out = {k: np.full(v.shape, np.nan) for k, v in coupled.items()}
    F = coupled["EE"].shape[0]
    for f in range(F):
        for g in (range(F) if cross else [f]):
            at = (f, g) if cross else (f,)
            ta = (g, f) if cross else (f,)
            x = solve_blocks(s4, [coupled[k][at] for k in ("EE", "EB", "BE", "BB")], act)
            for k, v in zip(("EE", "EB", "BE", "BB"), x):
                out[k][at] = v
            if "kk" in coupled:
                x = solve_blocks(s2, [coupled["kE"][at], coupled["kB"][at]], act)
                out["kE"][at], out["kB"][at] = x
                out["Ek"][ta], out["Bk"][ta] = x
                out["kk"][at] = solve_blocks(mats["M0"], [coupled["kk"][at]], act)[0]
    return out


def pcl_shear(fields, w, angle_deg, edges, cross=False):
    """The whole contract from the maps and the mask.  fields: a list of (gamma1, gamma2) or (gamma1, gamma2, kappa) f32
    maps.  dict: counts, coupled and cl (named arrays), spectra (per field the list E, B[, kappa]) and the matrices."""
    w = np.asarray(w, np.float32)
    n = w.shape[0]
    names = "EBk"[:len(fields[0])]
    spectra = []
    for fld in fields:
        g = [np.fft.rfft2((w * np.asarray(m, np.float32)).astype(np.float64)) for m in fld]
        spectra.append(list(rotate(g[0], g[1])) + g[2:])
    flat = [x for sp in spectra for x in sp]
    ref = power_np.power_of_spectra(flat, angle_deg, edges, cross=True)
    F, nc, B = len(fields), len(names), len(edges) - 1
    coupled = {}
    for a, la in enumerate(names):
        for b, lb in enumerate(names):
            v = np.empty((F, F, B) if cross else (F, B))
            for f in range(F):
                for g in (range(F) if cross else [f]):
                    v[(f, g) if cross else (f,)] = ref["cl"][f * nc + a, g * nc + b]
            coupled[la + lb] = v
    mats = matrices(w, edges)
    return {"counts": ref["counts"], "coupled": coupled, "cl": decouple(mats, coupled, ref["counts"], cross),
            "spectra": spectra, "matrices": mats, "n": n}
