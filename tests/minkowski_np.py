"""Restatement of the Minkowski-functional contract (include/slicer_amd.h) in numpy: ranks by
searchsorted in f64 with NaN -> 0, the map padded by one ring of rank 0, maxima and minima over shifted slices, bincount
and a reversed cumulative sum.  It imports nothing from the library."""
import numpy as np

KEYS = ("faces", "edges", "vertices", "boundary", "border", "euler", "nan")


def ranks(x, thresholds):
    """k(x): the number of thresholds <= x, the f32 pixels widened to f64; NaN -> 0."""
    t = np.asarray(thresholds, np.float64)
    v = np.asarray(x, np.float32).astype(np.float64)
    nan = np.isnan(v)
    k = np.searchsorted(t, np.where(nan, -np.inf, v), side="right")
    k[nan] = 0
    return k.astype(np.int64)


def above(values, T):
    """out[j] = the number of values > j, j = 0 ... T-1."""
    hist = np.bincount(np.asarray(values, np.int64).ravel(), minlength=T + 1)
    return np.cumsum(hist[::-1])[::-1][1:T + 1].astype(np.int64)


def counts(x, thresholds):
    """What Minkowski.read() returns for the map x."""
    x = np.asarray(x, np.float32)
    t = np.asarray(thresholds, np.float64)
    T = t.size
    k = ranks(x, t)
    p = np.pad(k, 1)  # positions outside the map are in no set
    vertex = np.maximum(np.maximum(p[:-1, :-1], p[:-1, 1:]), np.maximum(p[1:, :-1], p[1:, 1:]))  # (n+1)^2
    # horizontal edges lie between vertically adjacent faces (rows 0 and n: the rim), vertical ones likewise
    h_max, h_min = np.maximum(p[:-1, 1:-1], p[1:, 1:-1]), np.minimum(p[:-1, 1:-1], p[1:, 1:-1])  # [n+1, n]
    v_max, v_min = np.maximum(p[1:-1, :-1], p[1:-1, 1:]), np.minimum(p[1:-1, :-1], p[1:-1, 1:])  # [n, n+1]
    inner_max = above(np.concatenate([h_max[1:-1].ravel(), v_max[:, 1:-1].ravel()]), T)
    inner_min = above(np.concatenate([h_min[1:-1].ravel(), v_min[:, 1:-1].ravel()]), T)
    border = above(np.concatenate([h_max[0], h_max[-1], v_max[:, 0], v_max[:, -1]]), T)
    out = {"thresholds": t.copy(), "faces": above(k, T), "edges": inner_max + border, "vertices": above(vertex, T),
           "boundary": inner_max - inner_min, "border": border, "nan": int(np.isnan(x).sum())}
    out["euler"] = out["vertices"] - out["edges"] + out["faces"]
    return out


def same(got, ref):
    return all(np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)) for k in KEYS)
