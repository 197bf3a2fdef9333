"""What tests/test_xi_host.py and tests/test_gpu_xi.py share: the (n, L) cases with their edges,
the fields and the weight maps, and the direct pair sums of xi_np, computed once per (case, weights) and never changed."""
import functools
import math

import numpy as np

import xi_np

# (n, L, P, bins): the issue's table, then two cases named from the constants of slicer_xi.hip: (40, 32) has 2 L + 1 =
# 65 columns, one more than a k_xi_bin workgroup's kXiCols = 64 (so do (96, 40) and (97, 23) with a ragged second
# chunk; (33, 31) has 63, one fewer), and (40, 30) with 300 bins has more sums than one k_xi_sum workgroup's
# kSumThreads = 256.  bins = 0: the default edges below.
CASES = [(12, 11, 24, 0), (15, 13, 28, 0), (30, 15, 45, 0), (33, 31, 64, 0), (97, 23, 120, 0), (96, 40, 140, 0),
         (40, 32, 72, 0), (40, 30, 70, 300)]
WEIGHTS = ("none", "binary", "smooth", "corner")
# The reference figure: the largest error of the numpy FFT route against the direct sum, in units of U (xi_np.unit), as
# the issue measured it; test_xi_host re-measures and prints it.  The device bound is 16 times it.
REF_U = 0.36
DEVICE_U = 16 * REF_U


def edges_for(n, L, bins=0):
    """0, an exact integer radius (1, 2, 5), a bin with no lag (1.1 .. 1.3: no integer m2 in 1.21 .. 1.69), then
    steps up to L; the last edge of the case with L = n - 1 is sqrt(2) (n - 1), the farthest lag, in the closed bin."""
    last = math.sqrt(2.0) * (n - 1) if L == n - 1 else float(L)
    if bins:
        return np.linspace(0.0, last, bins + 1)
    e = [v for v in (0.0, 1.0, 1.1, 1.3, 2.0, 3.5, 5.0) if v < L - 1]
    e += [v for v in np.linspace(5.0, L, 5)[1:-1] if v > e[-1] + 0.5]
    return np.array(e + [last], np.float64)


@functools.lru_cache(maxsize=None)
def maps_for(n):
    """Four f32 maps of non-zero mean (a lost N(r) shows): smooth structure plus noise, each its own."""
    rng = np.random.default_rng(1800 + n)
    x = np.arange(n, dtype=np.float64)[:, None] / n
    y = np.arange(n, dtype=np.float64)[None, :] / n
    out = []
    for k in range(4):
        m = 0.7 - 0.3 * k + np.sin(2 * np.pi * ((k + 1) * x + 0.5 * k * y)) * np.cos(2 * np.pi * (k + 2) * y)
        m = m + 0.5 * rng.standard_normal((n, n))
        a = m.astype(np.float32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def weights_for(n, kind):
    if kind == "none":
        return None
    if kind == "binary":
        w = (np.random.default_rng(77 + n).random((n, n)) < 0.7).astype(np.float32)
    elif kind == "smooth":
        i = (np.arange(n, dtype=np.float64) + 0.5) / n
        w = ((0.2 + np.sin(np.pi * i)[:, None] ** 2) * (0.3 + np.cos(1.3 * i)[None, :] ** 2)).astype(np.float32)
    else:  # 1 on a 5 x 5 corner, 0 elsewhere
        w = np.zeros((n, n), np.float32)
        w[:5, :5] = 1.0
    w.setflags(write=False)
    return w


class Direct:
    """The direct pair sums of one (case, weights): C_ij(r) windows of the four maps, W(r), N_b, M_b."""

    def __init__(self, n, L, bins, kind):
        self.n, self.L = n, L
        self.edges = edges_for(n, L, bins)
        self.P = xi_np.padded_size(n, L)
        self.w = weights_for(n, kind)
        self.f = [xi_np.weighted(a, self.w) for a in maps_for(n)]
        self.norm = [float(np.sum(a * a)) for a in self.f]
        self.N, self.M = xi_np.enumerate_bins(n, self.edges)
        if self.w is None:
            self.Wwin, self.sumw2 = xi_np.pair_window(n, L), float(n * n)
        else:
            w64 = self.w.astype(np.float64)
            self.Wwin, self.sumw2 = xi_np.window(w64, w64, L), float(np.sum(w64 * w64))
        self.Wb, self.r = xi_np.weight_sums(self.Wwin, n, self.edges)
        self._c = {}

    def C(self, i, j):
        """The window of C_ij(r), maps i and j."""
        if i > j:
            return xi_np.flip(self.C(j, i))
        if (i, j) not in self._c:
            self._c[i, j] = xi_np.window(self.f[i], self.f[j], self.L)
        return self._c[i, j]

    def live(self):
        """The bins that are not empty: M_b > 0 and some pair of non-zero weight."""
        return (self.M > 0) & (self.Wb > 0)

    def spin0(self, i, j):
        """(xi_ij, U_b); NaN in the empty bins."""
        s = xi_np.bin_sum(self.C(i, j), self.n, self.edges)
        u = xi_np.unit(self.P, self.M, math.sqrt(self.norm[i] * self.norm[j]), self.Wb)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.live(), s / self.Wb, np.nan), u

    def spin2(self, a, b):
        """(xi+, xi-, U_b) of the spin-2 fields a = (i1, i2) and b = (j1, j2), map indices."""
        plus, minus = xi_np.spin2_sums(self.C(a[0], b[0]), self.C(a[1], b[1]), self.C(a[0], b[1]), self.C(a[1], b[0]),
                                       self.n, self.edges)
        na, nb = self.norm[a[0]] + self.norm[a[1]], self.norm[b[0]] + self.norm[b[1]]
        u = xi_np.unit(self.P, self.M, math.sqrt(na * nb), self.Wb)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.live(), plus / self.Wb, np.nan), np.where(self.live(), minus / self.Wb, np.nan), u


@functools.lru_cache(maxsize=None)
def direct(n, L, bins, kind):
    return Direct(n, L, bins, kind)


# the fields of the tests, as indices into maps_for: spin 0 takes three maps, spin 2 one or two (gamma1, gamma2) pairs
SPIN0 = (0, 1, 2)
SPIN2 = ((0, 1), (2, 3))


def pairs(F):
    return [(s, t) for s in range(F) for t in range(s, F)]
