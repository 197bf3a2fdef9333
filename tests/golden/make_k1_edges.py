"""Mines tests/golden/k1_edges.npz: raw f32 positions at the decision edges of the fast project+bin kernel.

Pure numpy on tests/np_restatement.py and tests/k1_edges_np.py, seeded, no GPU.  Run from the repository root:
    python tests/golden/make_k1_edges.py
The file holds, per fixture ("a": 512^2, slab bounds that are binary32 values; "b": 300^2, bounds that are not; "c":
300^2 at fov 0.5 and rcase 1 -- at depth 3 that field is wider than the box --, classes F and P only),
    <name>_params  Geometry.params()
    <name>_pos     [n, 3] f32 raw positions
    <name>_label   [n] uint16 class / detail bits (k1_edges_np.classify), recomputed by tests/test_k1_edges_host.py
How the classes are found (k1_edges_np has their definitions):
  T  map coordinates drawn log-uniformly in [2.5 / npix, 0.12] (fine f32 spacing: a tie every 2^-29 .. 2^-33) and
     uniformly over the map; whatever lies within 2^-41 of a tie is kept, everything within 2^-47 first.
  R  map coordinates drawn in the border rings.
  F  for random (y, z) the x that puts |dec| on the limit, and for random (x, y) the z that puts |ra| on it, are
     inverted approximately; the raw coordinate behind it is stepped +-4 f32 values and the candidates within 2^-41 kept.
  P  the F candidates that missed the window: inside the field, within 1e-6 relative of the limit.
  Z  the raw coordinate behind z is stepped +-64 f32 values around the inverse of every threshold.
  C  (300^2) as F, aimed at xs or ys = 0.25, 0.5, 0.75, 1: the only positive f32 values whose product with 300 is an
     integer.  At 0.75 the reference's floor(xs / dl) is one below the product (224 | 225); at the others they agree.
The binary32 slab set is 3.125 .. 3.875 and not 3, 3.25, ..: with rcase = 3 no transformed z lies below 3.0, so "one
f32 step below zlo[0]" would not exist.  3.9 is avoided in "b" (and 4.0 in "a") because that depth sits on the periodic
wrap of the raw coordinate for this centre.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import k1_edges_np as ke  # noqa: E402
import tile_np as tnp  # noqa: E402

F32, F64 = np.float32, np.float64
CENTER = (0.3, 0.6, 0.1)
GEOMS = {
    "a": ke.Geometry(512, 0.25, 1000.0, (-1, 1, -1), 3, CENTER, 3.0, [3.125, 3.3125, 3.5, 3.6875, 3.875]),
    "b": ke.Geometry(300, 0.25, 1000.0, (1, -1, 1), 5, CENTER, 3.0, [3.1, 3.3, 3.55, 3.7, 3.85]),
    "c": ke.Geometry(300, 0.5, 1000.0, (-1, -1, 1), 2, CENTER, 1.0, [1.1, 1.3, 1.55, 1.7, 1.85]),
}


def inverse(g, cx, cy, z):
    return tnp.raw_positions(cx, cy, z, g.box, g.rnd, g.fov)


def stepped(raw, axis, steps):
    """Every row of raw with its coordinate `axis` moved by -steps .. +steps f32 values."""
    k = np.arange(-steps, steps + 1, dtype=np.int32)
    out = np.repeat(raw, len(k), axis=0)
    col = np.ascontiguousarray(out[:, axis]).view(np.int32) + np.tile(k, len(raw))
    out[:, axis] = col.view(F32)
    return out


def zrange(g, rng, n):
    return rng.uniform(float(g.zb[0]) + 0.01, float(g.zb[-1]) - 0.01, n)


def take(raw, lab, bit, n, rng):
    i = np.nonzero(lab & bit)[0]
    return raw[i if len(i) <= n else rng.choice(i, n, replace=False)]


def mine_t(g, rng):
    lo = 2.5 / g.npix
    keep, below, above, rest = [], 0, 0, 0
    for it in range(40):
        m = 1 << 21
        if it % 4 == 3:
            cx, cy = rng.uniform(0.01, 0.99, m), rng.uniform(0.01, 0.99, m)
        else:
            cx, cy = (np.exp(rng.uniform(np.log(lo), np.log(0.12), m)) for _ in range(2))
        raw = inverse(g, cx, cy, zrange(g, rng, m))
        lab, _ = ke.classify(raw, g)
        for bit, cap in ((ke.T_BELOW, 96 - below), (ke.T_ABOVE, 96 - above)):
            keep.append(take(raw, lab, bit, max(cap, 0), rng))
        below += int(((lab & ke.T_BELOW) != 0).sum())
        above += int(((lab & ke.T_ABOVE) != 0).sum())
        far = ((lab & ke.T) != 0) & ((lab & (ke.T_BELOW | ke.T_ABOVE)) == 0)
        got = raw[far][:max(0, 360 - rest)] if it % 4 != 3 else raw[far]  # (every entry of the uniform draws)
        keep.append(got)
        rest += len(got)
        if below >= 80 and above >= 80 and rest >= 400:
            break
    return np.concatenate(keep)


def mine_r(g, rng):
    d, m = 1.0 / g.npix, 160
    out = []
    for ring in ((-d, d), (1 - d, 1 + d)):
        edge, free = rng.uniform(*ring, m), rng.uniform(0.02, 0.98, m)
        out += [inverse(g, edge, free, zrange(g, rng, m)), inverse(g, free, edge, zrange(g, rng, m))]
    raw = np.concatenate(out)
    lab, _ = ke.classify(raw, g)
    return raw[(lab & ke.R) != 0]


def mine_angle(g, rng, targets, m, want_bits, per_bit, with_p):
    """Candidates whose dec (then ra) lies next to fov * (target - 0.5) for every target: stepped along the raw
    coordinate behind x (behind y for ra)."""
    perm = tnp.FACE[g.face]
    out = []
    for axis in (0, 1):
        for t in targets:
            free = rng.uniform(0.15, 0.85, m)
            aim = np.full(m, t)
            raw = inverse(g, aim, free, zrange(g, rng, m)) if axis == 0 else inverse(g, free, aim, zrange(g, rng, m))
            cand = stepped(raw, perm[axis], 4)
            lab, _ = ke.classify(cand, g)
            for bit in want_bits:
                out.append(take(cand, lab, bit, per_bit, rng))
            if with_p:
                pure = cand[((lab & ke.P) != 0) & ((lab & ke.FC) == 0)]
                out.append(pure[rng.choice(len(pure), min(len(pure), 40), replace=False)])
    return np.concatenate(out)


def mine_z(g, rng):
    perm = tnp.FACE[g.face]
    out = []
    for b in g.zb:
        m = 48
        raw = inverse(g, rng.uniform(0.2, 0.8, m), rng.uniform(0.2, 0.8, m), np.full(m, float(b) - 1e-7))
        cand = stepped(raw, perm[2], 64)
        lab, e = ke.classify(cand, g)
        edge = ke.z_edge(e.z, g)
        for side in (0, 1):
            hit = np.nonzero(((lab & ke.Z) != 0) & (edge >= 0) & (edge % 2 == side) & (e.z.astype(F64) > b - 1e-5))[0]
            src = hit // 129  # one candidate per base particle
            _, first = np.unique(src, return_index=True)
            out.append(cand[hit[first][:8]])
    return np.concatenate(out)


def mine(name):
    g = GEOMS[name]
    rng = np.random.default_rng({"a": 20240511, "b": 20240512, "c": 20240513}[name])
    lim_s = float(g.lim / g.fov)
    parts = [mine_angle(g, rng, (0.5 - lim_s, 0.5 + lim_s), 1 << 19,
                        (ke.F_DEC_IN, ke.F_DEC_OUT, ke.F_RA_IN, ke.F_RA_OUT), 12, True)]
    if name != "c":
        parts += [mine_t(g, rng), mine_r(g, rng), mine_z(g, rng)]
    if name == "b":
        parts.append(mine_angle(g, rng, (0.25, 0.5, 0.75, 1.0), 64, (ke.C,), 12, False))
    raw = np.concatenate(parts).astype(F32)
    raw = np.unique(raw.view(np.uint32).reshape(-1, 3), axis=0).view(F32)
    # an entry within a few ulp64 of a tie rounds one way or the other with the last bit of the libm's asin / atan2:
    # its f32 coordinate would depend on the library, not on the arithmetic under test
    _, e = ke.classify(raw, g)
    raw = raw[np.minimum(np.abs(e.tdx), np.abs(e.tdy)) >= 2.0 ** -50]
    raw = raw[rng.permutation(len(raw))]
    lab, _ = ke.classify(raw, g)
    return g, np.ascontiguousarray(raw), lab


if __name__ == "__main__":
    out = {}
    for name in GEOMS:
        g, raw, lab = mine(name)
        out[name + "_params"], out[name + "_pos"], out[name + "_label"] = g.params(), raw, lab
        print(name, len(raw), {k: int(((lab & b) != 0).sum()) for k, b in
                               (("T", ke.T), ("T-", ke.T_BELOW), ("T+", ke.T_ABOVE), ("R", ke.R), ("F", ke.FC),
                                ("Fdi", ke.F_DEC_IN), ("Fdo", ke.F_DEC_OUT), ("Fri", ke.F_RA_IN), ("Fro", ke.F_RA_OUT),
                                ("Pd", ke.P_DEC), ("Pr", ke.P_RA), ("Z", ke.Z), ("C", ke.C), ("M", ke.M))})
    np.savez_compressed(os.path.join(HERE, "k1_edges.npz"), **out)
