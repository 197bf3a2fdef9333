"""The smoothing contract without a device: the restatement tests/smooth_np.py against a plain
Python loop (bit for bit), against scipy.ndimage.gaussian_filter (GAUSS) and a direct 2-D correlation with the sampled
aperture filter (MAP); the radius and tables of slicer_smooth_weights; that an implementation with f32 accumulators
would not pass a bitwise comparison; and the refusals of slicer_smooth_* that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import slicer_amd
import smooth_np as S
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6
CASES = ((64, 1.5), (100, 3.0), (257, 13.7))


def _err():
    return (L.slicer_last_error(None) or b"").decode()


def make_map(n, seed=0):
    rng = np.random.default_rng(104729 * n + seed)
    return (np.exp(rng.standard_normal((n, n))) - math.exp(0.5)).astype(np.float32)


def plain_tables(R, s):
    """Tables of any radius R for a scale s, in Python floats (the restatement takes its tables as arguments)."""
    q = [float(k * k) / (2.0 * (s * s)) for k in range(R + 1)]
    g = [math.exp(-v) for v in q]
    return g, [v * w for v, w in zip(q, g)]


def loop_line(v, w):
    """L_w of the list v, one output and one step at a time."""
    n, R = len(v), len(w) - 1
    at = lambda i: v[i] if 0 <= i < n else 0.0
    out = []
    for i in range(n):
        acc = w[0] * v[i]
        for k in range(1, R + 1):
            acc = acc + w[k] * (at(i - k) + at(i + k))
        out.append(acc)
    return out


def loop_axis0(rows, w):
    cols = [loop_line([r[j] for r in rows], w) for j in range(len(rows[0]))]
    return [[cols[j][i] for j in range(len(cols))] for i in range(len(rows))]


def loop_smooth(kind, x, g, h, s):
    n = x.shape[0]
    v = [[float(x[i, j]) for j in range(n)] for i in range(n)]
    out = np.empty((n, n), np.float32)
    if kind == "gauss":
        A = loop_axis0([loop_line(r, g) for r in v], g)
        N = loop_line([1.0] * n, g)
        for i in range(n):
            for j in range(n):
                out[i, j] = np.float32(A[i][j] / (N[i] * N[j]))
        return out
    G = [loop_line(r, g) for r in v]
    H = [loop_line(r, h) for r in v]
    D = [[a - b for a, b in zip(rg, rh)] for rg, rh in zip(G, H)]
    a, b = loop_axis0(D, g), loop_axis0(G, h)
    c = 1.0 / (((2.0 * math.pi) * s) * s)
    for i in range(n):
        for j in range(n):
            out[i, j] = np.float32(c * (a[i][j] - b[i][j]))
    return out


@pytest.mark.parametrize("R", [1, 2, 3, 12])
def test_restatement_is_the_plain_loop_bit_for_bit(R):
    s = R / 3.0 + 0.21
    g, h = plain_tables(R, s)
    for n in range(1, 10):
        x = make_map(n, R)
        for kind in ("gauss", "map"):
            got = S.smooth(kind, x, np.array(g), np.array(h), s)
            assert got.dtype == np.float32
            assert got.tobytes() == loop_smooth(kind, x, g, h, s).tobytes(), (n, R, kind)


@pytest.mark.parametrize("n,s", [(n, s) for n in (64, 100, 257) for s in (1.5, 3.0, 13.7)])
def test_gauss_restatement_agrees_with_scipy(n, s):
    from scipy import ndimage
    x = make_map(n)
    R, g, _ = slicer_amd.smooth_weights(s, 4.0)
    f = lambda a: ndimage.gaussian_filter(a, s, mode="constant", truncate=4.0)
    ref = f(x.astype(np.float64)) / f(np.ones((n, n), np.float64))
    err = float(np.abs(S.gauss(x, g).astype(np.float64) - ref).max()) / float(np.abs(ref).max())
    print(f"n = {n}, s = {s}, R = {R}: max|restatement - scipy| / max|scipy| = {err:.3g}")
    assert err <= 2.0 ** -23


def sampled_U(R, s):
    d = np.arange(-R, R + 1, dtype=np.float64)
    r2 = (d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * s * s)
    return (1.0 - r2) * np.exp(-r2) / (2.0 * np.pi * s * s)


@pytest.mark.parametrize("n,s,t", [(5, 1.5, 4.0), (16, 1.5, 4.0), (33, 1.5, 4.0), (16, 3.0, 4.0), (33, 3.0, 4.0), (33, 2.0, 5.0)])
def test_aperture_mass_restatement_is_the_direct_correlation(n, s, t):
    x = make_map(n)
    R, g, h = slicer_amd.smooth_weights(s, t)
    U = sampled_U(R, s)
    p = np.pad(x.astype(np.float64), R)
    direct = np.zeros((n, n), np.float64)
    for a in range(2 * R + 1):
        for b in range(2 * R + 1):
            direct += U[a, b] * p[a:a + n, b:b + n]
    got = S.aperture_mass64(x, g, h, s)
    bound = 1e-12 * float(np.abs(U).max()) * float(np.abs(x.astype(np.float64)).sum())
    err = float(np.abs(got - direct).max())
    print(f"n = {n}, s = {s}, R = {R}: max|restatement - direct| = {err:.3g}, bound {bound:.3g}")
    assert err <= bound
    spike = np.zeros((2 * R + 1, 2 * R + 1), np.float32)
    spike[R, R] = 1.0
    assert float(np.abs(S.aperture_mass(spike, g, h, s) - U).max()) <= 2.0 ** -23 * float(U.max())  # U is even


def test_weights_radius_is_scipys_rule():
    seen = set()
    grid = [(s, t) for s in (0.13, 0.3, 0.5, 1.0, 1.5, 2.5, 3.0, 8.0, 13.7, 16.0, 25.6, 32.0, 32.1)
            for t in (1.0, 2.0, 3.5, 4.0, 5.0, 8.0)]
    for m in (0, 1, 2, 7, 40, 127, 128):  # t s within 1e-12 of a half-integer
        for t in (1.0, 3.0, 4.0, 7.0):
            for d in (-1e-12, 0.0, 1e-12):
                grid.append(((m + 0.5 + d) / t, t))
    for s, t in grid:
        want = int(t * s + 0.5)
        R = C.c_int32(-1)
        rc = L.slicer_smooth_weights(s, t, C.byref(R), None, None)
        if want < 1:
            assert rc == ERR_ARG and "radius 0" in _err(), (s, t)
        elif want > 128:
            assert rc == ERR_UNSUPPORTED and "moments pyramid" in _err(), (s, t)
        else:
            assert rc == 0 and R.value == want, (s, t, R.value, want)
            assert slicer_amd.smooth_weights(s, t)[0] == want
        seen.add(min(max(want, 0), 129))
    assert {0, 1, 2, 3, 128, 129} <= seen and slicer_amd.SMOOTH_MAX_RADIUS == 128


@pytest.mark.parametrize("s,t", [(0.3, 4.0), (1.0, 4.0), (1.5, 4.0), (2.5, 4.0), (3.0, 5.0), (13.7, 4.0), (16.0, 8.0), (32.0, 4.0),
                                 (100.0, 1.0)])
def test_weights_tables(s, t):
    R, g, h = slicer_amd.smooth_weights(s, t)
    assert g.size == h.size == R + 1 and g[0] == 1.0 and h[0] == 0.0
    k = np.arange(R + 1, dtype=np.float64)
    q = (k * k) / (2.0 * (np.float64(s) * np.float64(s)))
    g_np = np.exp(-q)
    h_np = q * g_np
    assert np.all(np.abs(g - g_np) <= 2 * np.spacing(g_np)) and np.all(np.abs(h - h_np) <= 2 * np.spacing(h_np))
    assert np.all(np.diff(g) < 0) and np.all(g > 0)
    # any of the three outputs may be left out
    only_g = np.empty(R + 1)
    assert L.slicer_smooth_weights(s, t, None, only_g.ctypes.data, None) == 0 and only_g.tobytes() == g.tobytes()
    assert L.slicer_smooth_weights(s, t, None, None, None) == 0


def line_f32(v, w, axis):
    """smooth_np.line with f32 weights, values and accumulators."""
    w = np.asarray(w, np.float32)
    R, n = w.size - 1, v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (R, R)
    p = np.pad(v.astype(np.float32), pad)
    sh = lambda d: np.take(p, np.arange(R + d, R + d + n), axis=axis)
    acc = w[0] * sh(0)
    for k in range(1, R + 1):
        acc = acc + w[k] * (sh(-k) + sh(k))
    assert acc.dtype == np.float32
    return acc


@pytest.mark.parametrize("n,s", CASES)
def test_f32_accumulators_would_be_caught(n, s):
    x = make_map(n)
    _, g, h = slicer_amd.smooth_weights(s, 4.0)
    N = line_f32(np.ones(n, np.float32), g, 0)
    gauss32 = line_f32(line_f32(x, g, 1), g, 0) / (N[:, None] * N[None, :])
    G, H = line_f32(x, g, 1), line_f32(x, h, 1)
    map32 = np.float32(1.0 / (2.0 * np.pi * s * s)) * (line_f32(G - H, g, 0) - line_f32(G, h, 0))
    for kind, cheap in (("gauss", gauss32), ("map", map32)):
        ref = S.smooth(kind, x, g, h, s)
        differ = float(np.mean(cheap != ref))
        print(f"n = {n}, s = {s}, {kind}: {100 * differ:.1f} % of the pixels differ")
        assert differ > 0.5
        assert float(np.abs(cheap - ref).max()) <= 1e-4 * float(np.abs(ref).max())  # (it is the same filter)


@pytest.mark.parametrize("npix,kind,s,t,code,text", [
    (0, 0, 2.0, 4.0, ERR_ARG, "npix must be positive"),
    (-3, 1, 2.0, 4.0, ERR_ARG, "npix must be positive"),
    (131073, 0, 2.0, 4.0, ERR_UNSUPPORTED, "npix = 131073 above 131072"),
    (16, 2, 2.0, 4.0, ERR_ARG, "kind = 2 is neither SLICER_SMOOTH_GAUSS nor SLICER_SMOOTH_MAP"),
    (16, -1, 2.0, 4.0, ERR_ARG, "kind = -1 is neither SLICER_SMOOTH_GAUSS nor SLICER_SMOOTH_MAP"),
    (16, 0, 0.0, 4.0, ERR_ARG, "sigma_pix must be positive and finite"),
    (16, 1, -1.0, 4.0, ERR_ARG, "sigma_pix must be positive and finite"),
    (16, 0, math.nan, 4.0, ERR_ARG, "sigma_pix must be positive and finite"),
    (16, 0, math.inf, 4.0, ERR_ARG, "sigma_pix must be positive and finite"),
    (16, 0, 2.0, 0.99, ERR_ARG, "truncate must be within 1 ... 8"),
    (16, 1, 2.0, 8.01, ERR_ARG, "truncate must be within 1 ... 8"),
    (16, 0, 2.0, math.nan, ERR_ARG, "truncate must be within 1 ... 8"),
    (16, 0, 2.0, math.inf, ERR_ARG, "truncate must be within 1 ... 8"),
    (16, 0, 0.1, 4.0, ERR_ARG, "give the radius 0 (at least 1 pixel)"),
    (16, 1, 0.3, 1.0, ERR_ARG, "give the radius 0 (at least 1 pixel)"),
    (16, 0, 32.2, 4.0, ERR_UNSUPPORTED, "moments pyramid"),
    (131072, 1, 1e300, 8.0, ERR_UNSUPPORTED, "give a radius above 128 pixels"),
    (16, 0, 32.0, 4.0, ERR_ARG, "null argument"),  # R = 128 passes the numbers; there is no handle
    (131072, 1, 0.5, 1.0, ERR_ARG, "null argument"),
])
def test_create_refusals_need_no_device(npix, kind, s, t, code, text):
    out = C.c_void_p(1)
    assert L.slicer_smooth_create(None, npix, kind, s, t, C.byref(out)) == code
    assert _err().startswith("slicer_smooth_create: ") and text in _err(), _err()
    assert not out.value


def test_null_handles_and_the_python_wrappers_are_refused():
    buf = np.zeros(4, np.float32)
    p = C.c_void_p()
    assert L.slicer_smooth_run(None, buf.ctypes.data) == ERR_ARG and _err() == "slicer_smooth_run: null argument"
    assert L.slicer_smooth_run_npix(None, buf.ctypes.data, 1) == ERR_ARG and _err() == "slicer_smooth_run_npix: null argument"
    assert L.slicer_smooth_device_map(None, C.byref(p)) == ERR_ARG and _err() == "slicer_smooth_device_map: null argument"
    assert L.slicer_smooth_read(None, buf.ctypes.data) == ERR_ARG and _err() == "slicer_smooth_read: null argument"
    assert L.slicer_smooth_destroy(None) == ERR_ARG
    for s, t in ((0.1, 4.0), (40.0, 4.0), (1.0, 9.0), (math.nan, 4.0)):
        with pytest.raises(slicer_amd.SlicerError):
            slicer_amd.smooth_weights(s, t)
    with pytest.raises(ValueError):
        slicer_amd.Smooth(None, 16, kind="tophat", sigma_pix=2.0)
