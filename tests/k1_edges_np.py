"""Decision edges of the fast project+bin kernel (k_project_bin_fast), restated in numpy on np_restatement.

TEST INFRASTRUCTURE ONLY.  Shared by tests/golden/make_k1_edges.py (which mines tests/golden/k1_edges.npz),
tests/test_k1_edges_host.py (which recomputes every label of that file) and tests/test_gpu_project_bin_fast.py.

Everything is measured in f64 on the reference's own operation sequence (np_restatement.transform, then A3 of
np_restatement.select_project): s = ang / fov + 0.5 before its rounding to f32.  The distance of s from an f32
rounding tie comes from the low 29 bits of its f64 mantissa: the f32 neighbours of s differ in bit 29, the tie between
them is low29 == 2^28, and one unit of those bits is ulp64(s).
"""
import numpy as np

import np_restatement as npr

F32, F64 = np.float32, np.float64
WINDOW = 2.0 ** -41   # kMapWindow = kAngWindow of slicer_project_bin.hip
CLOSE = 2.0 ** -47    # the fast projection's own error budget
SLACK = 2.0 ** -46    # margin of the noted / clean predicates: twice that budget

# class bits of a particle's label
T, R, FC, P, Z, C, M = 1, 2, 4, 8, 16, 32, 64
# detail bits (label >> 8)
T_BELOW, T_ABOVE, F_DEC_IN, F_DEC_OUT, F_RA_IN, F_RA_OUT, P_DEC, P_RA = (1 << (8 + i) for i in range(8))


def ceil_to_f32(v):
    """Smallest f32 >= v (make_params pre-rounds the slab bounds this way: (double)z >= v <=> z >= ceil_to_f32(v))."""
    f = F32(v)
    return f if F64(f) >= F64(v) else np.nextafter(f, F32(np.inf))


def slab_bounds(edges, box):
    """f32 thresholds zlo[0..n-1], zlast of consecutive slabs with comoving bounds `edges` (n + 1 values)."""
    return np.array([ceil_to_f32(F64(e) / F64(box) * 1.e+3 / 1.0) for e in edges], F32)


def tie_distance(s):
    """Signed distance of f64 s from the nearest f32 rounding tie (negative: the tie lies above s in magnitude)."""
    s = np.ascontiguousarray(s, F64)
    bits = np.abs(s).view(np.uint64)
    low = (bits & np.uint64((1 << 29) - 1)).astype(np.int64) - (1 << 28)
    ex = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1023
    return low.astype(F64) * np.ldexp(1.0, (ex - 52).astype(np.int32))


class Geometry:
    def __init__(self, npix, fov, box, sgn, face, center, rcase, edges):
        self.npix, self.fov, self.box = int(npix), float(fov), float(box)
        self.sgn, self.face, self.rcase = tuple(int(s) for s in sgn), int(face), float(rcase)
        self.center = tuple(float(F32(c)) for c in center)
        self.edges = [float(e) for e in edges]
        self.lim = F64(self.fov) * (1. + 2. / self.npix) * 0.5
        self.zb = slab_bounds(self.edges, self.box)

    @property
    def rnd(self):
        return dict(sgn=self.sgn, face=self.face, center=self.center, rcase=self.rcase)

    def params(self):
        return np.array([self.npix, self.fov, self.box, *self.sgn, self.face, *self.center, self.rcase, *self.edges], F64)

    @staticmethod
    def from_params(p):
        return Geometry(int(p[0]), p[1], p[2], p[3:6], int(p[6]), p[7:10], p[10], p[11:])


class Entries:
    """Every particle of `raw` through transform and projection: f32 x, y, z; f64 dec, ra, sx, sy; plane (-1: in no
    slab), inside the field, selected."""

    def __init__(self, raw, g):
        self.g = g
        self.x, self.y, self.z = npr.transform(raw, g.box, g.sgn, g.face, g.center, g.rcase)
        X, Y, Zd = self.x.astype(F64) - 0.5, self.y.astype(F64) - 0.5, self.z.astype(F64)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.sqrt(X * X + Y * Y + Zd * Zd)
            self.dec, self.ra = np.arcsin(X / d), np.arctan2(Y, Zd)
        self.sx, self.sy = self.dec / F64(g.fov) + 0.5, self.ra / F64(g.fov) + 0.5
        self.xs, self.ys = self.sx.astype(F32), self.sy.astype(F32)
        p = np.zeros(len(self.z), np.int64) - 1
        for k in range(len(g.zb) - 1):
            p[self.z >= g.zb[k]] = k
        p[self.z >= g.zb[-1]] = -1
        self.plane = p
        self.inside = (np.abs(self.ra) <= g.lim) & (np.abs(self.dec) <= g.lim)
        self.selected = self.inside & (p >= 0)
        self.tdx, self.tdy = tie_distance(self.sx), tie_distance(self.sy)


def pretest_outside(e, g, margin=True):
    """The kernel's conservative f32 pre-test of the FOV cut with the constants of k1_fast_args (margin=False: k_ra
    without its 3e-5 margin and eps_ra = 0).  z * k is exact in f64, so with eps = 0 the sum below rounds once, as the
    kernel's fmaf does.

    Without the margin the ra test still rejects no selected entry, whatever the geometry: |ra| <= lim means
    |Y| <= Z tan(lim) <= z k with k = ceil_to_f32(tan lim), and rounding to nearest is monotonic, so
    fl32(|y - 0.5|) <= fl32(z k).  The margin of k_ra is slack, not a condition of correctness; class M (selected
    entries that only the margin keeps) is therefore empty, which tests/test_k1_edges_host.py asserts on the entries
    next to the limit."""
    tl = np.tan(g.lim)
    k_ra = ceil_to_f32(tl * (1.0 + 3e-5)) if margin else ceil_to_f32(tl)
    eps_ra = F32(2e-6) if margin else F32(0)
    k_dec = ceil_to_f32(tl * np.sqrt(1.0 + F64(k_ra) * F64(k_ra)) * (1.0 + 3e-5))
    eps_dec = ceil_to_f32(tl * 2.2e-6 + 1e-6)
    z = e.z.astype(F64)
    lim_ra = (z * F64(k_ra) + F64(eps_ra)).astype(F32)
    lim_dec = (z * F64(k_dec) + F64(eps_dec)).astype(F32)
    return (np.abs(e.y - F32(0.5)) > lim_ra) | (np.abs(e.x - F32(0.5)) > lim_dec)


def _ring(s, npix):
    d = 1.0 / npix
    return ((s >= -d) & (s <= d)) | ((s >= 1 - d) & (s <= 1 + d))


def classify(raw, g):
    """uint16 label per particle: class bits T R FC P Z C, detail bits above them."""
    e = Entries(raw, g)
    lab = np.zeros(len(e.z), np.uint16)
    ring = _ring(e.sx, g.npix) | _ring(e.sy, g.npix)
    # T: a map coordinate within the window of an f32 rounding tie, away from the border rings
    td = np.where(np.abs(e.tdx) <= np.abs(e.tdy), e.tdx, e.tdy)
    t = e.selected & ~ring & (np.abs(td) <= WINDOW)
    lab[t] |= T
    lab[t & (np.abs(td) <= CLOSE) & (td < 0)] |= T_BELOW
    lab[t & (np.abs(td) <= CLOSE) & (td > 0)] |= T_ABOVE
    lab[e.selected & ring] |= R
    # F: an angle within the window of the FOV limit while the other angle is well inside (the decision shows)
    slab = e.plane >= 0
    ddec, dra = np.abs(e.dec) - g.lim, np.abs(e.ra) - g.lim
    fdec = slab & (np.abs(ddec) <= WINDOW) & (dra < -1e-3)
    fra = slab & (np.abs(dra) <= WINDOW) & (ddec < -1e-3)
    lab[fdec | fra] |= FC
    lab[fdec & (ddec <= 0)] |= F_DEC_IN
    lab[fdec & (ddec > 0)] |= F_DEC_OUT
    lab[fra & (dra <= 0)] |= F_RA_IN
    lab[fra & (dra > 0)] |= F_RA_OUT
    # P: inside the field within 1e-6 relative of the limit: the f32 pre-test must let it through
    pdec = e.selected & (ddec <= 0) & (ddec >= -1e-6 * g.lim)
    pra = e.selected & (dra <= 0) & (dra >= -1e-6 * g.lim)
    lab[pdec | pra] |= P
    lab[pdec] |= P_DEC
    lab[pra] |= P_RA
    # M: selected entries that only the margin of k_ra keeps (none: see pretest_outside)
    lab[e.selected & pretest_outside(e, g, margin=False) & ~pretest_outside(e, g, margin=True)] |= M
    # Z: inside the field, z on a slab threshold or one f32 step below it
    lab[e.inside & (z_edge(e.z, g) >= 0)] |= Z
    # C: an entry exactly on a cell boundary
    tx, ty = e.xs.astype(F64) * g.npix, e.ys.astype(F64) * g.npix
    lab[e.selected & ((tx == np.floor(tx)) | (ty == np.floor(ty)))] |= C
    return lab, e


def z_edge(z, g):
    """2 k + side for z == zb[k] (side 0) or its lower f32 neighbour (side 1); -1 elsewhere."""
    out = np.zeros(len(z), np.int64) - 1
    for k, b in enumerate(g.zb):
        out[z == b] = 2 * k
        out[z == np.nextafter(b, F32(0))] = 2 * k + 1
    return out


def note_state(e, g, series_max):
    """What decide_emit does with every entry that reaches it, from the kernel's documented conditions and its error
    budget: +1 it is certainly noted for the exact epilogue, 0 it is certainly decided by the fast code, -1 either may
    happen (within the fast projection's own error of a window's end)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        X, Y, Zd = e.x.astype(F64) - 0.5, e.y.astype(F64) - 0.5, e.z.astype(F64)
        tn, sn = np.abs(Y / Zd), np.abs(X / np.sqrt(Y * Y + Zd * Zd))
    dist = [np.abs(e.tdx), np.abs(e.tdy), np.abs(np.abs(e.dec) - g.lim), np.abs(np.abs(e.ra) - g.lim)]
    sure = (dist[0] <= WINDOW - SLACK) | (dist[1] <= WINDOW - SLACK) | (dist[2] <= WINDOW - SLACK) | \
           (dist[3] <= WINDOW - SLACK) | (sn > series_max * 1.001) | (tn > series_max * 1.001)
    maybe = (dist[0] <= WINDOW + SLACK) | (dist[1] <= WINDOW + SLACK) | (dist[2] <= WINDOW + SLACK) | \
            (dist[3] <= WINDOW + SLACK) | (sn > series_max * 0.999) | (tn > series_max * 0.999)
    if not g.npix & (g.npix - 1) == 0:  # not a power of two: an entry exactly on a cell boundary is noted
        tx, ty = e.xs.astype(F64) * g.npix, e.ys.astype(F64) * g.npix
        sure = sure | (tx == np.floor(tx)) | (ty == np.floor(ty))
        # (xs one f32 step off decides the cell of an entry the fast code rounds correctly only when decided: covered
        #  by the tie window above)
    return np.where(sure, 1, np.where(maybe, -1, 0))
