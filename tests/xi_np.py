"""f64 numpy restatement of the real-space two-point contract, written from its formulas.

Fields are f32 maps a of n^2 pixels, axis 0 slow; one weight map w (None: 1) is shared; a~ = a * w in f64 (exact).  For
a lag r = (dx, dy) != 0 along (axis 0, axis 1): C_ab(r) = sum_x a~(x) b~(x + r) over the x with both pixels inside the
map, W(r) the same of w with itself, N(r) = (n - |dx|)(n - |dy|).  A lag is in bin b iff RN64(r_b^2) <= m2 <
RN64(r_{b+1}^2) on the integer m2 = dx^2 + dy^2, the last bin closed, m2 = 0 in none.  Three forms:
  the direct pair sum over slices, one lag at a time (lag_sum, window)
  the numpy FFT route: zero padding to P >= n + L, rfft2, products, irfft2 (window_fft)
  a brute-force spin-2 form that rotates every pair into (gamma_t, gamma_x) explicitly (brute_spin2)."""
import math

import numpy as np


def supported(p):
    """A size the f64 transform plans: 2 <= p <= 16384 with prime factors 2, 3, 5, 7 only."""
    if p < 2 or p > 16384:
        return False
    for q in (2, 3, 5, 7):
        while p % q == 0:
            p //= q
    return p == 1


def max_lag(n, edges):
    return min(int(math.ceil(float(edges[-1]))), n - 1)


def padded_size(n, L):
    """The smallest supported P >= n + L, or 0."""
    for p in range(n + L, 16385):
        if supported(p):
            return p
    return 0


def bin_index(m2, edges):
    """Bin of every integer m2 (any shape), -1: in no bin."""
    e2 = np.asarray(edges, np.float64) ** 2
    B = e2.size - 1
    m2 = np.asarray(m2)
    x = m2.astype(np.float64)
    b = np.searchsorted(e2, x, side="right") - 1
    b = np.where((b == B) & (x == e2[B]), B - 1, b)
    b = np.where((b < 0) | (b >= B) | (m2 == 0), -1, b)
    return b


def lag_grid(L):
    """dx, dy [2L+1, 2L+1] of the window, index [dx + L, dy + L]."""
    d = np.arange(-L, L + 1, dtype=np.int64)
    return np.meshgrid(d, d, indexing="ij")


def enumerate_bins(n, edges):
    """(N_b, M_b) int64 by enumeration of every lag of the window."""
    L = max_lag(n, edges)
    dx, dy = lag_grid(L)
    b = bin_index(dx * dx + dy * dy, edges)
    B = len(edges) - 1
    keep = b >= 0
    pairs = (n - np.abs(dx)) * (n - np.abs(dy))
    N = np.zeros(B, np.int64)
    np.add.at(N, b[keep], pairs[keep])
    return N, np.bincount(b[keep], minlength=B).astype(np.int64)


def weighted(a, w):
    a = np.asarray(a, np.float32).astype(np.float64)
    return a if w is None else a * np.asarray(w, np.float32).astype(np.float64)


def lag_sum(a, b, dx, dy):
    """sum_x a(x) b(x + (dx, dy)) over the x with both pixels inside, a and b f64 [n, n]."""
    n = a.shape[0]
    x0, x1 = max(0, -dx), min(n, n - dx)
    y0, y1 = max(0, -dy), min(n, n - dy)
    return float(np.sum(a[x0:x1, y0:y1] * b[x0 + dx:x1 + dx, y0 + dy:y1 + dy]))


def window(a, b, L):
    """C_ab(r) for every lag of the window [2L+1, 2L+1] by lag_sum, one lag at a time (C at r = 0 included)."""
    out = np.empty((2 * L + 1, 2 * L + 1))
    same = a is b
    for dx in range(-L, L + 1):
        for dy in range(-L, L + 1):
            if same and (dx < 0 or (dx == 0 and dy < 0)):
                continue  # C_aa(-r) = C_aa(r): the same products
            out[dx + L, dy + L] = lag_sum(a, b, dx, dy)
    if same:
        flip = out[::-1, ::-1]
        dxg, dyg = lag_grid(L)
        neg = (dxg < 0) | ((dxg == 0) & (dyg < 0))
        out[neg] = flip[neg]
    return out


def window_fft(a, b, L, P):
    """The same by the FFT route: zero padding to P^2, irfft2(conj(rfft2 a) rfft2 b), lags at (dx mod P, dy mod P)."""
    n = a.shape[0]
    pa, pb = np.zeros((P, P)), np.zeros((P, P))
    pa[:n, :n], pb[:n, :n] = a, b
    c = np.fft.irfft2(np.conj(np.fft.rfft2(pa)) * np.fft.rfft2(pb), s=(P, P))
    idx = np.arange(-L, L + 1) % P
    return c[np.ix_(idx, idx)]


def pair_window(n, L):
    """N(r) of the window, exact integers as f64."""
    dx, dy = lag_grid(L)
    return ((n - np.abs(dx)) * (n - np.abs(dy))).astype(np.float64)


def spin4(L):
    """c4, s4 [2L+1, 2L+1] from the integer lags (0 at r = 0)."""
    dx, dy = lag_grid(L)
    x, y = dx.astype(np.float64), dy.astype(np.float64)
    m4 = (x * x + y * y) ** 2
    m4[L, L] = 1.0
    return (x ** 4 - 6.0 * x * x * y * y + y ** 4) / m4, 4.0 * x * y * (x * x - y * y) / m4


def bin_sum(win, n, edges):
    """The sum of a window's values per bin, [B]."""
    L = (win.shape[0] - 1) // 2
    dx, dy = lag_grid(L)
    b = bin_index(dx * dx + dy * dy, edges)
    keep = b >= 0
    return np.bincount(b[keep], weights=win[keep], minlength=len(edges) - 1)


def weight_sums(Wwin, n, edges):
    """W_b and r_mean_b (NaN where W_b is 0) of the window W(r)."""
    L = (Wwin.shape[0] - 1) // 2
    dx, dy = lag_grid(L)
    Wb = bin_sum(Wwin, n, edges)
    Wr = bin_sum(Wwin * np.sqrt((dx * dx + dy * dy).astype(np.float64)), n, edges)
    with np.errstate(invalid="ignore", divide="ignore"):
        return Wb, np.where(Wb > 0, Wr / Wb, np.nan)


def flip(win):
    """C_ba(r) = C_ab(-r)."""
    return win[::-1, ::-1]


def spin2_windows(c11, c22, c12, c21):
    """The three windows of a spin-2 pair: C_11 + C_22, C_11 - C_22, C_12 + C_21."""
    return c11 + c22, c11 - c22, c12 + c21


def spin2_sums(c11, c22, c12, c21, n, edges):
    """(sum of C_11 + C_22, sum of (C_11 - C_22) c4 + (C_12 + C_21) s4) per bin: xi+ W_b and xi- W_b."""
    L = (c11.shape[0] - 1) // 2
    c4, s4 = spin4(L)
    plus, minus, cross = spin2_windows(c11, c22, c12, c21)
    return bin_sum(plus, n, edges), bin_sum(minus * c4 + cross * s4, n, edges)


def brute_spin2(a1, a2, b1, b2, w, edges):
    """xi+ W_b and xi- W_b of the spin-2 fields a = (a1, a2), b = (b1, b2) pair by pair: gamma_t + i gamma_x =
    -gamma e^(-2 i phi), phi = atan2(dy, dx), xi+- = sum w w' (gt gt' +- gx gx').  O(n^4): small n only."""
    n = np.asarray(a1).shape[0]
    ga = weighted(a1, w) + 1j * weighted(a2, w)
    gb = weighted(b1, w) + 1j * weighted(b2, w)
    B = len(edges) - 1
    plus, minus = np.zeros(B), np.zeros(B)
    L = max_lag(n, edges)
    for x0 in range(n):
        for y0 in range(n):
            for x1 in range(max(0, x0 - L), min(n, x0 + L + 1)):
                for y1 in range(max(0, y0 - L), min(n, y0 + L + 1)):
                    dx, dy = x1 - x0, y1 - y0
                    b = int(bin_index(np.int64(dx * dx + dy * dy), edges))
                    if b < 0:
                        continue
                    rot = -np.exp(-2j * math.atan2(dy, dx))
                    p, q = ga[x0, y0] * rot, gb[x1, y1] * rot
                    plus[b] += p.real * q.real + p.imag * q.imag
                    minus[b] += p.real * q.real - p.imag * q.imag
    return plus, minus


def unit(P, lags, norm, Wb=None):
    """U_b = 2^-52 log2(P) M_b norm / W_b (no division for W_b itself: Wb = None).  norm: the sum of a~^2 over the field's
    components, the geometric mean of the two fields' sums for a cross pair, or the sum of w^2."""
    u = 2.0 ** -52 * math.log2(P) * np.asarray(lags, np.float64) * float(norm)
    if Wb is None:
        return u
    with np.errstate(invalid="ignore", divide="ignore"):
        return u / np.asarray(Wb, np.float64)
