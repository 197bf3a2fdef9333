"""Restatement of the PDF-histogram and peak / minimum-count contract (include/slicer_amd.h) in
numpy: bins by searchsorted in f64 with the closed last bin and the outside counts, peaks and minima from the eight
shifted slices of the interior.  It imports nothing from the library."""
import numpy as np


def uniform_edges(lo, hi, bins):
    """e_0 = lo, e_B = hi, e_b = lo + b * ((hi - lo) / B) between, every operation rounded once to f64."""
    lo, hi = np.float64(lo), np.float64(hi)
    width = (hi - lo) / np.float64(bins)
    e = lo + np.arange(bins + 1, dtype=np.float64) * width
    e[0], e[bins] = lo, hi
    return e


def histogram(values, edges):
    """(counts int64 [B], below, above, nan) of f32 values widened to f64 against the f64 edges."""
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    v = np.asarray(values, np.float32).astype(np.float64).ravel()
    nan = np.isnan(v)
    v = v[~nan]
    below, above = v < edges[0], v > edges[B]
    b = np.searchsorted(edges, v[~below & ~above], "right") - 1
    b[b == B] = B - 1  # x = e_B: the closed last bin
    return np.bincount(b, minlength=B).astype(np.int64), int(below.sum()), int(above.sum()), int(nan.sum())


def extrema(x):
    """(peak mask, minimum mask) of the interior x[1:-1, 1:-1]: strictly greater / less than each of the 8 neighbours,
    compared in f32.  Comparisons with NaN are false.  For n < 3 the masks are empty."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    if n < 3:
        return np.zeros((0, 0), bool), np.zeros((0, 0), bool)
    c = x[1:-1, 1:-1]
    peak, minimum = np.ones(c.shape, bool), np.ones(c.shape, bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            nb = x[1 + di:n - 1 + di, 1 + dj:n - 1 + dj]
            peak &= c > nb
            minimum &= c < nb
    return peak, minimum


def counts(x, edges, masks=None):
    """What Peaks.read() returns for the map x; masks: extrema(x) where the caller already has it."""
    x = np.asarray(x, np.float32)
    edges = np.asarray(edges, np.float64)
    peak, minimum = extrema(x) if masks is None else masks
    inner = x[1:-1, 1:-1] if x.shape[0] >= 3 else np.zeros((0, 0), np.float32)
    out = {"edges": edges.copy(), "below": np.zeros(3, np.int64), "above": np.zeros(3, np.int64)}
    for k, (name, v) in enumerate((("pdf", x), ("peaks", inner[peak]), ("minima", inner[minimum]))):
        out[name], out["below"][k], out["above"][k], nan = histogram(v, edges)
        if k == 0:
            out["nan"] = nan
    return out
