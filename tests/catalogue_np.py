"""Restatement of the peak / minimum catalogue contract (include/slicer_amd.h) in numpy: the
extrema are those of tests/peaks_np.py, the selection is in f64, the refinement is the least-squares quadratic of the
3 x 3 window in f64, one numpy operation per rounding in the order the contract states.  It imports nothing from the
library."""
import numpy as np

import peaks_np as P

DTYPE = np.dtype([("row", "<i4"), ("col", "<i4"), ("value", "<f4"), ("flags", "<u4"), ("dy", "<f8"), ("dx", "<f8")])
PEAKS, MINIMA = 1, 2      # kinds
MINIMUM, FALLBACK = 1, 2  # flags


def window_terms(z):
    """(gy, gx, hyy, hxx, hxy) of windows z[..., 3, 3] (f64; z[..., a + 1, b + 1] is row offset a, column offset b)."""
    z = np.asarray(z, np.float64)
    R = [(z[..., a, 0] + z[..., a, 1]) + z[..., a, 2] for a in range(3)]
    Cs = [(z[..., 0, b] + z[..., 1, b]) + z[..., 2, b] for b in range(3)]
    gy = (R[2] - R[0]) / 6.0
    gx = (Cs[2] - Cs[0]) / 6.0
    hyy = ((R[2] + R[0]) - 2.0 * R[1]) / 3.0
    hxx = ((Cs[2] + Cs[0]) - 2.0 * Cs[1]) / 3.0
    hxy = ((z[..., 2, 2] + z[..., 0, 0]) - (z[..., 2, 0] + z[..., 0, 2])) / 4.0
    return gy, gx, hyy, hxx, hxy


def refine(z, minimum):
    """(dy, dx, accepted, why) of windows z[K, 3, 3]; minimum[K]: bool.  why: 0 accepted, else the first rule that
    failed: 1 det <= 0 (or NaN), 2 the sign of hyy, 3 an offset that is not finite, 4 an offset beyond 0.5."""
    with np.errstate(all="ignore"):
        gy, gx, hyy, hxx, hxy = window_terms(z)
        det = hyy * hxx - hxy * hxy
        dy = -((hxx * gy - hxy * gx) / det)
        dx = -((hyy * gx - hxy * gy) / det)
        curved = np.where(minimum, hyy > 0.0, hyy < 0.0)
        finite = np.isfinite(dy) & np.isfinite(dx)
        near = (np.abs(dy) <= 0.5) & (np.abs(dx) <= 0.5)
    why = np.select([~(det > 0.0), ~curved, ~finite, ~near], [1, 2, 3, 4], 0)
    ok = why == 0
    return np.where(ok, dy, 0.0), np.where(ok, dx, 0.0), ok, why


def windows(x, rows, cols):
    """The 3 x 3 windows of x about (rows, cols), [K, 3, 3] in f64."""
    x = np.asarray(x, np.float32)
    z = np.empty((len(rows), 3, 3), np.float64)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            z[:, a + 1, b + 1] = x[rows + a, cols + b]
    return z


def catalogue(x, kinds=PEAKS | MINIMA, min_peak=-np.inf, max_minimum=np.inf, with_why=False):
    """Every record of the map x under the selection, in ascending row * n + col (no capacity); with_why: also refine's
    reason per record."""
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    peak, minimum = P.extrema(x)
    inner = x[1:-1, 1:-1].astype(np.float64) if n >= 3 else np.zeros((0, 0))
    peak = peak & bool(kinds & PEAKS) & (inner >= np.float64(min_peak))
    minimum = minimum & bool(kinds & MINIMA) & (inner <= np.float64(max_minimum))
    rows, cols = np.nonzero(peak | minimum)  # row-major: ascending row * n + col
    is_min = minimum[rows, cols]
    rows, cols = rows + 1, cols + 1
    dy, dx, ok, why = refine(windows(x, rows, cols), is_min)
    rec = np.zeros(len(rows), DTYPE)
    rec["row"], rec["col"], rec["value"] = rows, cols, x[rows, cols]
    rec["flags"] = np.where(is_min, MINIMUM, 0) | np.where(ok, 0, FALLBACK)
    rec["dy"], rec["dx"] = dy, dx
    return (rec, why) if with_why else rec


def totals(rec):
    """(kept peaks, kept minima) of records."""
    m = int(np.count_nonzero(rec["flags"] & MINIMUM))
    return len(rec) - m, m
