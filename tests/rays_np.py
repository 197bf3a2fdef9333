"""numpy restatement of the multi-plane ray tracer (the contract is stated in
include/slicer_amd.h), in f64 in the stated order, and a plain per-ray loop over Python floats that says the same.
Imports nothing from the library.

Every numpy operation on f64 arrays is one IEEE operation rounded once, and so is every operation on Python floats, so
the two agree bit for bit, and with the device.  NaN: where a result is NaN its sign and payload are not part of the
contract (same_bits below compares NaN as equal to NaN)."""
import math

import numpy as np

STATE = ("b1", "b2", "t1", "t2", "A11", "A12", "A21", "A22", "T11", "T12", "T21", "T22")
B1, B2, T1, T2, A11, A12, A21, A22, T11, T12, T21, T22 = range(12)
KAPPA, GAMMA1, GAMMA2, OMEGA, DEFLECTION1, DEFLECTION2 = range(6)
BIG = 2.0 ** 30


def same_bits(a, b):
    """True if a and b (same dtype, f32 or f64) agree bit for bit, a NaN of any kind matching a NaN of any kind."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def weight(chi, chi_last):
    """w = RN(RN(chi - chi_last) / chi) of Python floats."""
    return (float(chi) - float(chi_last)) / float(chi)


def start(n):
    """[12, n, n] f64: b = t = (i - h, j - h), A = T = I."""
    h = (n - 1) / 2.0
    s = np.zeros((12, n, n), np.float64)
    i = np.arange(n, dtype=np.float64)
    s[B1] = s[T1] = (i - h)[:, None]
    s[B2] = s[T2] = (i - h)[None, :]
    s[A11] = s[A22] = s[T11] = s[T22] = 1.0
    return s


def _advance(x, y, w):
    return x + w * (y - x)


def step(s, w, d, maps):
    """The state after the plane whose five f32 [n, n] maps are maps = (alpha1, alpha2, kappa, gamma1, gamma2)."""
    n = s.shape[1]
    h = (n - 1) / 2.0
    s = s.copy()
    with np.errstate(all="ignore"):
        for x, y in ((B1, T1), (B2, T2), (A11, T11), (A12, T12), (A21, T21), (A22, T22)):
            s[x] = _advance(s[x], s[y], w)
        u1, u2 = s[B1] + h, s[B2] + h
        ok = (np.abs(u1) < BIG) & (np.abs(u2) < BIG)  # False for NaN and the infinities too
        fl1, fl2 = np.floor(np.where(ok, u1, 0.0)), np.floor(np.where(ok, u2, 0.0))
        f1 = np.where(ok, u1 - fl1, np.nan)
        f2 = np.where(ok, u2 - fl2, np.nan)
        g1, g2 = 1.0 - f1, 1.0 - f2
        lo1, lo2 = np.mod(fl1.astype(np.int64), n), np.mod(fl2.astype(np.int64), n)
        hi1, hi2 = np.mod(lo1 + 1, n), np.mod(lo2 + 1, n)
        v = []
        for m in maps:
            m = np.asarray(m, np.float32).astype(np.float64)
            r0 = g2 * m[lo1, lo2] + f2 * m[lo1, hi2]
            r1 = g2 * m[hi1, lo2] + f2 * m[hi1, hi2]
            v.append(g1 * r0 + f1 * r1)
        va1, va2, vk, vg1, vg2 = v
        U11, U22, U12 = vk + vg1, vk - vg1, vg2
        s[T1] = s[T1] - va1 / d
        s[T2] = s[T2] - va2 / d
        t11 = s[T11] - (U11 * s[A11] + U12 * s[A21])
        t12 = s[T12] - (U11 * s[A12] + U12 * s[A22])
        t21 = s[T21] - (U12 * s[A11] + U22 * s[A21])
        t22 = s[T22] - (U12 * s[A12] + U22 * s[A22])
        s[T11], s[T12], s[T21], s[T22] = t11, t12, t21, t22
    return s


def observe(s, w, d):
    """[6, n, n] f32: kappa, gamma1, gamma2, omega, deflection1, deflection2 for the source weight w."""
    n = s.shape[1]
    h = (n - 1) / 2.0
    i = np.arange(n, dtype=np.float64)
    th1 = np.broadcast_to((i - h)[:, None], (n, n))
    th2 = np.broadcast_to((i - h)[None, :], (n, n))
    with np.errstate(all="ignore"):
        b1, b2 = _advance(s[B1], s[T1], w), _advance(s[B2], s[T2], w)
        a11, a12 = _advance(s[A11], s[T11], w), _advance(s[A12], s[T12], w)
        a21, a22 = _advance(s[A21], s[T21], w), _advance(s[A22], s[T22], w)
        out = [1.0 - 0.5 * (a11 + a22), 0.5 * (a22 - a11), -0.5 * (a12 + a21), 0.5 * (a21 - a12), (th1 - b1) * d,
               (th2 - b2) * d]
        return np.stack([o.astype(np.float32) for o in out])


def trace(n, d, chis, planes, chi_s=None):
    """Through the planes (each five f32 maps) at the distances chis: the state, and the outputs at chi_s if given."""
    s, last = start(n), 0.0
    for chi, maps in zip(chis, planes):
        s = step(s, weight(chi, last), d, maps)
        last = float(chi)
    return s if chi_s is None else (s, observe(s, weight(chi_s, last), d))


# ---- the same, ray by ray, over Python floats ----

def _f32(x):
    """RN of a Python float to f32, as a Python float."""
    with np.errstate(all="ignore"):
        return float(np.float32(x))


def _div(a, b):
    """IEEE a / b of Python floats (b != 0 here; Python raises on a zero divisor, IEEE does not)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def scalar_trace(n, d, chis, planes, chi_s):
    """trace() as a plain loop: ([12, n, n] f64 state, [6, n, n] f32 outputs)."""
    h = (n - 1) / 2.0
    state = np.zeros((12, n, n), np.float64)
    out = np.zeros((6, n, n), np.float32)
    planes = [[np.asarray(m, np.float32) for m in maps] for maps in planes]
    for i in range(n):
        for j in range(n):
            b1 = t1 = i - h
            b2 = t2 = j - h
            a11 = a22 = T11_ = T22_ = 1.0
            a12 = a21 = T12_ = T21_ = 0.0
            last = 0.0
            for chi, maps in zip(chis, planes):
                w = (float(chi) - last) / float(chi)
                last = float(chi)
                b1 = b1 + w * (t1 - b1)
                b2 = b2 + w * (t2 - b2)
                a11 = a11 + w * (T11_ - a11)
                a12 = a12 + w * (T12_ - a12)
                a21 = a21 + w * (T21_ - a21)
                a22 = a22 + w * (T22_ - a22)
                u1, u2 = b1 + h, b2 + h
                if abs(u1) < BIG and abs(u2) < BIG:
                    fl1, fl2 = math.floor(u1), math.floor(u2)
                    f1, f2 = u1 - fl1, u2 - fl2
                    lo1, lo2 = fl1 % n, fl2 % n  # Python's % is the mathematical modulo
                else:
                    f1 = f2 = math.nan
                    lo1 = lo2 = 0
                hi1, hi2 = (lo1 + 1) % n, (lo2 + 1) % n
                g1, g2 = 1.0 - f1, 1.0 - f2
                v = []
                for m in maps:
                    m00, m01 = float(m[lo1, lo2]), float(m[lo1, hi2])
                    m10, m11 = float(m[hi1, lo2]), float(m[hi1, hi2])
                    r0 = g2 * m00 + f2 * m01
                    r1 = g2 * m10 + f2 * m11
                    v.append(g1 * r0 + f1 * r1)
                va1, va2, vk, vg1, vg2 = v
                U11, U22, U12 = vk + vg1, vk - vg1, vg2
                t1 = t1 - _div(va1, d)
                t2 = t2 - _div(va2, d)
                n11 = T11_ - (U11 * a11 + U12 * a21)
                n12 = T12_ - (U11 * a12 + U12 * a22)
                n21 = T21_ - (U12 * a11 + U22 * a21)
                n22 = T22_ - (U12 * a12 + U22 * a22)
                T11_, T12_, T21_, T22_ = n11, n12, n21, n22
            state[:, i, j] = (b1, b2, t1, t2, a11, a12, a21, a22, T11_, T12_, T21_, T22_)
            w = (float(chi_s) - last) / float(chi_s)
            s1, s2 = b1 + w * (t1 - b1), b2 + w * (t2 - b2)
            o11, o12 = a11 + w * (T11_ - a11), a12 + w * (T12_ - a12)
            o21, o22 = a21 + w * (T21_ - a21), a22 + w * (T22_ - a22)
            vals = (1.0 - 0.5 * (o11 + o22), 0.5 * (o22 - o11), -0.5 * (o12 + o21), 0.5 * (o21 - o12),
                    ((i - h) - s1) * d, ((j - h) - s2) * d)
            out[:, i, j] = [_f32(x) for x in vals]
    return state, out


def noise_planes(rng, n, n_planes, d, shift_pixels=3.0, lens=0.3):
    """White-noise planes: deflections of a few pixels (so that rays wrap on small grids), kappa and shear of `lens`."""
    planes = []
    for _ in range(n_planes):
        a = [(rng.standard_normal((n, n)) * shift_pixels * d).astype(np.float32) for _ in range(2)]
        k = [(rng.standard_normal((n, n)) * lens).astype(np.float32) for _ in range(3)]
        planes.append(a + k)
    return planes


# ---- whole- and half-pixel shifts, whose answer is known exactly ----

D = 2.0 ** -12  # a spacing that keeps products with small integers exact


def quantised_plane(rng, n):
    """alpha in multiples of d / 16, kappa and shear in multiples of 2^-10: with d a power of two every operation of
    the tracer on them is exact, so the expected values below do not depend on the order they are formed in."""
    a = [(rng.integers(-64, 65, (n, n)) * (D / 16)).astype(np.float32) for _ in range(2)]
    k = [(rng.integers(-300, 301, (n, n)) / 1024.0).astype(np.float32) for _ in range(3)]
    return a + k


def shifted(m, s1, s2):
    """m read at (i - s1, j - s2), bilinearly and periodically, for shifts that are whole or half pixels: the exact
    average of the one, two or four samples."""
    m = np.asarray(m, np.float64)
    rows = [int(np.floor(s1))] if s1 == np.floor(s1) else [int(np.floor(s1)), int(np.floor(s1)) + 1]
    cols = [int(np.floor(s2))] if s2 == np.floor(s2) else [int(np.floor(s2)), int(np.floor(s2)) + 1]
    return sum(np.roll(m, (r, c), axis=(0, 1)) for r in rows for c in cols) / (len(rows) * len(cols))


def shift_case(n, s1, s2, seed=0):
    """Planes at chi = 1, 2 and a source at 4: plane 1 deflects every ray by (2 s1, 2 s2) pixels, so that the rays meet
    plane 2 displaced by (-s1, -s2).  Returns the planes and the six expected outputs."""
    rng = np.random.default_rng(seed + n)
    zero = np.zeros((n, n), np.float32)
    p1 = [np.full((n, n), 2 * s1 * D, np.float32), np.full((n, n), 2 * s2 * D, np.float32), zero, zero, zero]
    p2 = quantised_plane(rng, n)
    a1, a2, k, g1, g2 = (shifted(m, s1, s2) for m in p2)
    U11, U22, U12 = k + g1, k - g1, g2
    A11, A22, A12 = 1 - 0.5 * U11, 1 - 0.5 * U22, 0 - 0.5 * U12  # A = I - U / 2, entry by entry
    ref = [1 - 0.5 * (A11 + A22), 0.5 * (A22 - A11), -0.5 * (A12 + A12), 0.5 * (A12 - A12), 1.5 * s1 * D + 0.5 * a1,
           1.5 * s2 * D + 0.5 * a2]
    return [p1, p2], np.stack(ref).astype(np.float32)
