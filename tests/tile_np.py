"""Restatement of the tile deposit's accounting (k_build_items, k_tile_deposit) and exact per-pixel sums, in numpy and
Python integers.  TEST INFRASTRUCTURE ONLY: tests/test_gpu_tile_deposit.py derives its bounds from it, and
tests/test_tile_bound_host.py keeps those bounds honest without a GPU.

Every f32 contribution c of np_restatement.tsc_contributions is a multiple of 2^-149; with 2^le above the largest mass
(le <= 10: MAX_M = 1e3 < 2^10) it is split exactly into four 40-bit limbs in units of 2^(le-40), 2^(le-80), 2^(le-120),
2^(le-160); the limbs are summed per pixel in int64 (< 2^23 terms) and joined as Python integers.  E, the exact sum of a
pixel, is therefore an integer number of UNIT = 2^(le-160), and every bound below is compared in integers.

J, the number of addends the design lets reach a pixel's global cell (DESIGN.md S3 "accumulator contracts"): summed over
the tile launches of the pass and over the (plane, tile) bins whose records touch the pixel, the number of parts of that
bin in that launch -- 1 while the bin stays whole (up to WHOLE_RECS records, WHOLE_RECS_INT in a launch with integer
cells), ceil(tot / ITEM_RECS) beyond -- plus, with integer cells, the contributions that are no multiple of the tile's
quantum 2^(le-49) and go straight to the global map.
"""
import numpy as np

F32, F64 = np.float32, np.float64
ITEM_RECS = 16384
WHOLE_RECS = 65536      # f64, fixed-point and count cells
WHOLE_RECS_INT = 32768  # integer cells: N * 0.5625 * 2^49 < 2^64 needs N <= 58254
FACE = {1: (0, 1, 2), 2: (0, 2, 1), 3: (1, 2, 0), 4: (1, 0, 2), 5: (2, 0, 1), 6: (2, 1, 0)}


def raw_positions(xs, ys, z, box, rnd, fov):
    """Raw box positions whose projection lands near the map coordinates (xs, ys) in [0, 1) at transformed depth z (box
    units, rcase included).  Only approximately the inverse of oracle.transform / select_project (f32 positions): the
    callers project forward with the oracle and select by what they get."""
    xs, ys, z = (np.asarray(a, F64) for a in (xs, ys, z))
    Y = z * np.tan((ys - 0.5) * fov)
    X = np.sqrt(Y * Y + z * z) * np.tan((xs - 0.5) * fov)
    out = [X + 0.5, Y + 0.5, z - float(rnd["rcase"])]
    perm = FACE[int(rnd["face"])]
    raw = np.empty((len(xs), 3), F64)
    for a in range(3):
        b = np.mod(out[a] + float(rnd["center"][a]), 1.0)  # out[a] = wrap(b[perm[a]] - centre[a])
        raw[:, perm[a]] = np.mod(float(rnd["sgn"][perm[a]]) * b, 1.0) * box
    return raw.astype(F32)


def mass_le(mmax):
    """2^le above the largest (capped) mass, as make_params / k_tile_deposit take it from the f32 exponent."""
    mmax = float(F32(mmax))
    return int(np.frexp(mmax)[1]) if mmax > 0 else 0  # frexp: m = f * 2^e, 0.5 <= f < 1  ->  e = ilogb(m) + 1


def cap_mass(m):
    m = np.asarray(m, F32)
    return np.where(m > F32(1000.0), F32(0), m).astype(F32)


def parts_of(tot, int_cells):
    tot = np.asarray(tot, np.int64)
    whole = WHOLE_RECS_INT if int_cells else WHOLE_RECS
    return np.where(tot <= whole, (tot > 0).astype(np.int64), (tot + ITEM_RECS - 1) // ITEM_RECS)


def _group_sum(keys, order, starts, v):
    return np.add.reduceat(v[order], starts) if len(keys) else np.zeros(0, v.dtype)


class Pixels:
    """Exact sums and counts of the contributions (pix [n, 9] with -1 = clipped, val [n, 9] f32) per pixel."""

    def __init__(self, pix, val, npix, le):
        self.npix, self.le = npix, le
        ok = pix >= 0
        self.p = pix[ok]
        self.v = val[ok].astype(F64)
        self.rec = np.broadcast_to(np.arange(pix.shape[0])[:, None], pix.shape)[ok]
        self.order = np.argsort(self.p, kind="stable")
        ps = self.p[self.order]
        self.starts = np.nonzero(np.r_[True, ps[1:] != ps[:-1]])[0] if len(ps) else np.zeros(0, np.int64)
        self.upix = ps[self.starts] if len(ps) else np.zeros(0, np.int64)

    def count(self, mask=None):
        """Per touched pixel: number of contributions (of those in mask)."""
        w = np.ones(len(self.p), np.int64) if mask is None else mask.astype(np.int64)
        return _group_sum(self.upix, self.order, self.starts, w)

    def exact(self):
        """Per touched pixel: E as a Python integer number of 2^(le - 160)."""
        r = self.v.copy()
        E = np.zeros(len(self.upix), object)
        for j in range(4):
            unit = np.ldexp(1.0, self.le - 40 * (j + 1))
            limb = np.floor(r / unit)
            r = r - limb * unit
            s = _group_sum(self.upix, self.order, self.starts, limb.astype(np.int64))
            E = E + s.astype(object) * (1 << (40 * (3 - j)))
        assert not r.any(), "a contribution below 2^(le-160): not an f32 value"
        return E

    def fixed(self, e):
        """Per touched pixel: sum of rint(c * 2^e) (int64), the FIXED64 accumulator."""
        t = self.v * np.ldexp(1.0, e)
        assert float(t.max(initial=0.0)) < 2.0 ** 52
        return _group_sum(self.upix, self.order, self.starts, np.rint(t).astype(np.int64))

    def units(self, a):
        """f32 / f64 values at the touched pixels -> Python integers in units of 2^(le - 160)."""
        x = np.asarray(a, F64).reshape(-1)[self.upix] * np.ldexp(1.0, 160 - self.le)
        assert np.all(x == np.floor(x))
        return np.array([int(t) for t in x], object)

    def full(self, per_pixel, dtype):
        out = np.zeros(self.npix * self.npix, dtype)
        out[self.upix] = per_pixel
        return out.reshape(self.npix, self.npix)


def not_quantum(val, le):
    """Contributions that are no multiple of the integer cells' quantum 2^(le-49): they bypass the tile."""
    t = val.astype(F64) * np.ldexp(1.0, 49 - le)
    return t != np.rint(t)


def noted_records(val, m, le):
    """Records the branch-free loop notes: the smallest of the nine products (clipped ones included, as in the kernel)
    below 2^(le-25); records of mass 0 (capped ones too) are skipped before the test."""
    return (val.min(axis=1) < F32(np.ldexp(1.0, le - 25))) & (np.asarray(m, F32) != 0)


def addends(P, pix, val, rec_bin, rec_launch, int_cells):
    """J per touched pixel (module docstring) and the parts of every (launch, bin) as a dict."""
    key = rec_launch.astype(np.int64) * (1 << 20) + rec_bin.astype(np.int64)
    ukey, inv, tot = np.unique(key, return_inverse=True, return_counts=True)
    nparts = parts_of(tot, int_cells)
    ok = pix >= 0
    ckey = np.broadcast_to(inv[:, None], pix.shape)[ok]
    cval = val[ok]
    direct = not_quantum(cval, P.le) if int_cells else np.zeros(len(cval), bool)
    in_tile = (cval != 0) & ~direct
    # distinct (launch, bin, pixel) among the contributions that reach an LDS cell
    trip = np.unique(ckey[in_tile].astype(np.int64) * (P.npix * P.npix) + P.p[in_tile])
    J = np.zeros(P.npix * P.npix, np.int64)
    np.add.at(J, trip % (P.npix * P.npix), nparts[trip // (P.npix * P.npix)])
    np.add.at(J, P.p[direct], 1)
    return J[P.upix], {int(k): int(n) for k, n in zip(ukey, nparts)}


def _rn32(n, ex):
    """Round-to-nearest-even of n * 2^ex to f32 (n >= 0), normal range."""
    if n == 0:
        return F32(0)
    drop = max(n.bit_length() - 24, -149 - ex, 0)  # (f32 values are multiples of 2^-149)
    if drop > 0:
        q, r = n >> drop, n & ((1 << drop) - 1)
        half = 1 << (drop - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        return F32(np.ldexp(float(q), ex + drop))
    return F32(np.ldexp(float(n), ex))


# ---- emulation of one pixel's journey (tests/test_tile_bound_host.py) ---------------------------------------------
def emulate_pixel(c, part_of, cells, le):
    """One pixel's value in the F32 mode from contributions c (f32), dealt to work items part_of[i] (0 .. J-1): every
    item sums its share in an LDS cell of kind `cells` -- "int" (exact multiples of 2^(le-49)), "f64", or "f32" (what
    the design rules out) -- and adds one value, rounded to f32, to the global f32 cell in item order."""
    g = F32(0)
    for j in range(int(part_of.max()) + 1):
        mine = c[part_of == j]
        if cells == "int":
            t = mine.astype(F64) * np.ldexp(1.0, 49 - le)
            assert np.all(t == np.rint(t))
            s = sum(int(x) for x in t)
            assert s < 1 << 64, "integer cell wrapped"
            flush = _rn32(s, le - 49)
        elif cells == "f64":
            s = F64(0)
            for x in mine:
                s = F64(s + F64(x))
            flush = F32(s)
        else:
            s = F32(0)
            for x in mine:
                s = F32(s + x)
            flush = s
        g = F32(g + flush)
    return g
