"""numpy restatement of slicer_smooth_* (DESIGN.md S8 row N12), operation for operation in f64.  It imports nothing from
the library: the weight tables g, h (slicer_smooth_weights) are arguments.

Line operator L_w along one axis, samples outside the map taken as +0.0:
    acc_0 = w_0 v[i];  acc_k = acc_{k-1} + w_k (v[i-k] + v[i+k]),  k = 1 ... R, from the centre outwards,
every operation a whole-array numpy f64 operation, so each is rounded once and nothing is fused."""
import numpy as np


def line(v, w, axis):
    """L_w of the f64 array v along `axis`."""
    v = np.asarray(v, np.float64)
    w = np.asarray(w, np.float64)
    R, n = w.size - 1, v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (R, R)
    p = np.pad(v, pad)  # zeros: +0.0

    def shifted(d):
        return p[(slice(None),) * axis + (slice(R + d, R + d + n),)]

    acc = w[0] * shifted(0)
    for k in range(1, R + 1):
        acc = acc + w[k] * (shifted(-k) + shifted(k))
    return acc


def norm(n, g):
    """N[i]: L_g of a line of n ones, the weight of the filter that lies inside the map about sample i."""
    return line(np.ones(n, np.float64), g, 0)


def gauss64(x, g):
    """The Gaussian-smoothed map in f64, before its rounding to f32."""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        T = line(x, g, 1)
        A = line(T, g, 0)
        N = norm(x.shape[0], g)
        return A / (N[:, None] * N[None, :])


def gauss(x, g):
    with np.errstate(over="ignore", invalid="ignore"):
        return gauss64(x, g).astype(np.float32)


def aperture_mass64(x, g, h, s):
    """The aperture-mass map in f64, before its rounding to f32."""
    x = np.asarray(x, np.float32).astype(np.float64)
    s = np.float64(s)
    with np.errstate(invalid="ignore", over="ignore"):
        G = line(x, g, 1)
        H = line(x, h, 1)
        D = G - H
        a = line(D, g, 0)
        b = line(G, h, 0)
        c = np.float64(1.0) / (((np.float64(2.0) * np.float64(np.pi)) * s) * s)
        return c * (a - b)


def aperture_mass(x, g, h, s):
    with np.errstate(over="ignore", invalid="ignore"):
        return aperture_mass64(x, g, h, s).astype(np.float32)


def smooth(kind, x, g, h, s):
    return gauss(x, g) if kind == "gauss" else aperture_mass(x, g, h, s)
