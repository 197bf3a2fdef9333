"""Restatement of the Betti-number contract (include/slicer_amd.h) with scipy.ndimage.label: ranks
as minkowski_np.ranks, beta_0 the 8-connected components of every set {k > j} (the 3 x 3 structure), beta_1 the
4-connected components (the cross) of the complement padded by one ring of True, minus the one that holds the ring.  It
imports nothing from the library."""
import numpy as np
from scipy import ndimage

KEYS = ("components", "holes", "faces", "nan")
EIGHT = np.ones((3, 3), bool)
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def ranks(x, thresholds):
    """k(x): the number of thresholds <= x, the f32 pixels widened to f64; NaN -> 0."""
    t = np.asarray(thresholds, np.float64)
    v = np.asarray(x, np.float32).astype(np.float64)
    nan = np.isnan(v)
    k = np.searchsorted(t, np.where(nan, -np.inf, v), side="right")
    k[nan] = 0
    return k.astype(np.int64)


def of_set(q):
    """(components, holes) of one boolean set q."""
    components = ndimage.label(q, structure=EIGHT)[1]
    outside_and_holes = ndimage.label(np.pad(~q, 1, constant_values=True), structure=FOUR)[1]
    return components, outside_and_holes - 1


def counts(x, thresholds):
    """What Betti.read() returns for the map x.  A threshold whose rank no pixel has leaves the set of the next one
    unchanged, and its labelling is not repeated."""
    x = np.asarray(x, np.float32)
    t = np.asarray(thresholds, np.float64)
    T = t.size
    k = ranks(x, t)
    hist = np.bincount(k.ravel(), minlength=T + 1)
    components, holes, faces = (np.zeros(T, np.int64) for _ in range(3))
    for j in range(T - 1, -1, -1):
        if j < T - 1 and hist[j + 1] == 0:  # Q_j = Q_{j+1}
            components[j], holes[j], faces[j] = components[j + 1], holes[j + 1], faces[j + 1]
            continue
        q = k > j
        components[j], holes[j] = of_set(q)
        faces[j] = int(q.sum())
    return {"thresholds": t.copy(), "components": components, "holes": holes, "faces": faces, "nan": int(np.isnan(x).sum())}


def same(got, ref):
    return all(np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64)) for k in KEYS)
