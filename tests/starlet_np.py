"""numpy restatement of slicer_starlet_* and slicer_l1norm_* (DESIGN.md S8 row N16), in the operation order of
include/slicer_amd.h.  It imports nothing from the library.

Starlet: whole-array f64 operations on np.take with the mirror index; numpy rounds every array operation once and fuses
nothing, so the values are those of the contract.  l1norm: the bin rule of tests/peaks_np.py's PDF and math.fsum, the
exact sum rounded once."""
import math

import numpy as np


def refl(i, n):
    """The mirror index about the edge pixels, which are not repeated; i: any integer array."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)  # non-negative
    return np.where(m < n, m, p - m)


def line(v, d, axis):
    """A_d along `axis` of the f64 array v."""
    n = v.shape[axis]
    i = np.arange(n, dtype=np.int64)
    t = lambda o: np.take(v, refl(i + o, n), axis=axis)
    a = t(-d) + t(d)
    b = t(-2 * d) + t(2 * d)
    return (((6.0 * v) + (4.0 * a)) + b) * 0.0625


def starlet(x, scales):
    """[coarse, w_1, ..., w_J], f32 each, of the f32 map x."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] == x.shape[1]
    c = x.astype(np.float64)
    w = []
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(scales):
            d = 1 << j
            c1 = line(line(c, d, 1), d, 0)
            w.append((c - c1).astype(np.float32))
            c = c1
        return [c.astype(np.float32)] + w


def reach(x, scales):
    """Per output [coarse, w_1 ... w_J] the boolean map of the pixels that a non-finite input pixel reaches: those whose
    value depends on one, by the supports of the definition (a w_j depends on c_{j-1} at the pixel and on c_j)."""
    bad = ~np.isfinite(np.asarray(x))
    n = bad.shape[0]
    i = np.arange(n, dtype=np.int64)
    out = []
    for j in range(scales):
        d = 1 << j
        nxt = bad
        for axis in (1, 0):
            nxt = np.logical_or.reduce([np.take(nxt, refl(i + o, n), axis=axis) for o in (-2 * d, -d, 0, d, 2 * d)])
        out.append(bad | nxt)
        bad = nxt
    return [bad] + out


def gains(scales):
    """(gain_w [J], gain_coarse) in long double by the definition: H_0 = delta, H_j = H_{j-1} * (1, 4, 6, 4, 1) / 16 dilated
    by 2^{j-1}, gain_j = sqrt(sum_ab (H_{j-1}[a] H_{j-1}[b] - H_j[a] H_j[b])^2) over the full 2-D tables."""
    ld = np.longdouble
    h = np.array([1], dtype=object)  # exact integers over 16^j
    out = []
    for j in range(1, scales + 1):
        d = 1 << (j - 1)
        nxt = np.zeros(h.size + 4 * d, dtype=object)
        for t, tap in enumerate((1, 4, 6, 4, 1)):
            nxt[t * d:t * d + h.size] += h * tap
        prev = np.zeros(nxt.size, dtype=object)
        prev[2 * d:2 * d + h.size] = h * 16
        unit = ld(16) ** ld(-j)
        p = np.array([ld(int(v)) for v in prev]) * unit
        q = np.array([ld(int(v)) for v in nxt]) * unit
        diff = np.outer(p, p) - np.outer(q, q)
        out.append(np.sqrt((diff * diff).sum()))
        h = nxt
    coarse = np.sqrt((np.outer(q, q) ** 2).sum())
    return np.array(out, dtype=ld), coarse


def l1norm(x, edges):
    """dict: counts [B], l1 [B] (math.fsum of |x| widened, per bin), below, above, nan, below_l1, above_l1."""
    v = np.asarray(x, np.float32).ravel().astype(np.float64)
    e = np.asarray(edges, np.float64)
    B = e.size - 1
    nan = np.isnan(v)
    below = ~nan & (v < e[0])
    above = ~nan & (v > e[B])
    inside = ~nan & ~below & ~above
    # the number of e_0 ... e_{B-1} that are <= x, minus one: x = e_B falls into the last bin
    b = np.searchsorted(e[:B], v[inside], side="right") - 1
    a = np.abs(v)
    order = np.argsort(b, kind="stable")
    cuts = np.searchsorted(b[order], np.arange(B + 1))
    vals = a[inside][order]
    with np.errstate(invalid="ignore"):
        l1 = np.array([_fsum(vals[cuts[k]:cuts[k + 1]]) for k in range(B)], np.float64)
    return {"counts": np.diff(cuts).astype(np.int64), "l1": l1, "below": int(below.sum()), "above": int(above.sum()),
            "nan": int(nan.sum()), "below_l1": _fsum(a[below]), "above_l1": _fsum(a[above])}


def _fsum(values):
    return math.inf if np.isinf(values).any() else math.fsum(values.tolist())
