"""Non-finite and out-of-domain particles for the deposit path: the value classes, where they go, and the pools.
TEST INFRASTRUCTURE ONLY: tests/test_hostile_particles_host.py checks the classes against the oracle and the second
restatement without a GPU; tests/test_gpu_hostile_particles.py feeds them to every route of the device path.

Values are kept as f32 BIT PATTERNS (uint32) from the table to the device: a signalling NaN does not survive a trip
through a Python float (the f32 -> f64 conversion quiets it).

A position class replaces ONE raw coordinate of a particle that the oracle otherwise selects (BASES: mid-field of both
settings).  Two settings (face 3 with signs (-1, 1, -1); face 5 with the opposite signs) give every raw axis two of the
three roles and both signs, and every role -- x, y, z -- two raw axes and both signs:
    setting 0:  x = +raw[1]   y = -raw[2]   z = -raw[0]
    setting 1:  x = +raw[2]   y = +raw[0]   z = -raw[1]
What the oracle does with a class is one of
    S   quiet (guard silent), the particle is selected in one of the four slabs
    D   quiet, the particle is dropped (slab test or field of view)
    G   the negativity guard fires (createDensityMaps returns 1)
and OUTCOMES holds it for every (class, setting, raw axis) as a literal: a class cannot change sides without notice.
"""
import numpy as np

import oracle
from slicer_amd import synth

F32 = np.float32
BOX = 1000.0
SLABS4 = [3.0, 3.25, 3.5, 3.75, 4.0]  # four consecutive slabs of one box replication (rcase 3)
FOV = 0.25
CENTER = tuple(float(F32(c)) for c in (0.3, 0.6, 0.1))  # f32 values: the fast project+bin kernel qualifies
SETTINGS = [dict(sgn=(-1, 1, -1), face=3, center=CENTER, rcase=3.0),
            dict(sgn=(1, -1, 1), face=5, center=CENTER, rcase=3.0)]
BASES = [(520.0, 770.0, 930.0), (130.0, 520.0, 770.0)]  # raw positions near the map centre at z ~ 3.4, per setting


def bits_of(v):
    return int(np.array([v], F32).view(np.uint32)[0])


def _next(v, towards):
    return np.nextafter(F32(v), F32(towards))


_B = F32(BOX)
_Q100 = F32(np.ldexp(BOX, -100))  # box 2^-100: the quotient r / box sits at 2^-100, the kQLo end of the fast kernel's sweep
INF = F32(np.inf)
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny

POSITION_CLASSES = {
    "qnan+": 0x7FC00000, "qnan-": 0xFFC00000, "qnan payload": 0x7FC12345, "0x7F800001": 0x7F800001,
    "+inf": bits_of(INF), "-inf": bits_of(-INF), "+FLT_MAX": bits_of(FLT_MAX), "-FLT_MAX": bits_of(-FLT_MAX),
    "+1e30": bits_of(1e30), "-1e30": bits_of(-1e30),
    "box": bits_of(_B), "box-": bits_of(_next(_B, 0)), "box+": bits_of(_next(_B, INF)), "2 box": bits_of(2 * BOX),
    "2.5 box": bits_of(2.5 * BOX), "-0.1 box": bits_of(-0.1 * BOX), "-2.6 box": bits_of(-2.6 * BOX), "-0.0": 0x80000000,
    "denormal min+": 0x00000001, "denormal min-": 0x80000001, "denormal max+": 0x007FFFFF, "denormal max-": 0x807FFFFF,
    "FLT_MIN": bits_of(FLT_MIN),
    "box 2^-100": bits_of(_Q100), "box 2^-100 -": bits_of(_next(_Q100, 0)), "box 2^-100 +": bits_of(_next(_Q100, INF)),
    "box 2^-126": bits_of(np.ldexp(BOX, -126)),
}

MASS_CLASSES = {
    "nan+": 0x7FC00000, "nan-": 0xFFC00000, "-1": bits_of(-1.0), "-2^-10": bits_of(-2.0 ** -10), "+0.0": 0, "-0.0": 0x80000000,
    "+inf": bits_of(INF), "-inf": bits_of(-INF),
    "1000": bits_of(1000.0), "1000-": bits_of(_next(1000.0, 0)), "1000+": bits_of(_next(1000.0, INF)),
    "FLT_MAX": bits_of(FLT_MAX), "denormal min": 0x00000001, "denormal max": 0x007FFFFF, "FLT_MIN": bits_of(FLT_MIN),
    "2^-100": bits_of(2.0 ** -100),
}
# what a TSC map does with the class (oracle/slicer_oracle.c: orc_select_project caps, orc_gridist_w takes the root):
# "nan" the 3x3 footprint becomes NaN; "zero" nothing but +0 is added; "kept" the mass is deposited
MASS_TSC = {"nan+": "nan", "nan-": "nan", "-1": "nan", "-2^-10": "nan", "-inf": "nan",
            "+0.0": "zero", "-0.0": "zero", "+inf": "zero", "1000+": "zero", "FLT_MAX": "zero",
            "1000": "kept", "1000-": "kept", "denormal min": "kept", "denormal max": "kept", "FLT_MIN": "kept",
            "2^-100": "kept"}
POISON_MASSES = [k for k, v in MASS_TSC.items() if v == "nan"]

# (class) -> outcome on raw axis 0, 1, 2 in setting 0, then in setting 1.  Generated once with outcome() below, kept as
# a literal; tests/test_hostile_particles_host.py recomputes it.
OUTCOMES = {
    "qnan+": "DDD DDD", "qnan-": "DDD DDD", "qnan payload": "DDD DDD", "0x7F800001": "DDD DDD",
    # the wrap subtracts or adds 1 once: a huge value stays huge, and its sign after the axis' mirror decides --
    # negative trips the guard, positive fails the slab test (z) or the field of view (x, y)
    "+inf": "GDG DGD", "-inf": "DGD GDG", "+FLT_MAX": "GDG DGD", "-FLT_MAX": "DGD GDG", "+1e30": "GDG DGD",
    "-1e30": "DGD GDG",
    "box": "SSS SSS", "box-": "SSS SSS", "box+": "SSS SSS",
    "2 box": "DSG SDS", "2.5 box": "DSG SDS", "-0.1 box": "SSS SSS", "-2.6 box": "SGD GSG", "-0.0": "SSS SSS",
    "denormal min+": "SSS SSS", "denormal min-": "SSS SSS", "denormal max+": "SSS SSS", "denormal max-": "SSS SSS",
    "FLT_MIN": "SSS SSS", "box 2^-100": "SSS SSS", "box 2^-100 -": "SSS SSS", "box 2^-100 +": "SSS SSS",
    "box 2^-126": "SSS SSS",
}


def mass_values(names):
    return np.array([MASS_CLASSES[k] for k in names], np.uint32).view(F32)


def class_particles(setting, classes=None):
    """One particle per (class, raw axis): BASES[setting] with that coordinate replaced.  -> labels [(class, axis)],
    positions [n, 3] f32."""
    labels = [(c, a) for c in (classes if classes is not None else POSITION_CLASSES) for a in range(3)]
    pos = np.tile(np.array(BASES[setting], F32).view(np.uint32), (len(labels), 1))
    for i, (c, a) in enumerate(labels):
        pos[i, a] = POSITION_CLASSES[c]
    return labels, pos.view(F32)


def outcome(pos, setting, npix=512):
    """'S', 'D' or 'G' per particle of pos, each taken alone, from the oracle (guard: any transformed coordinate < 0)."""
    r = SETTINGS[setting]
    x, y, z = oracle.transform(pos, BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    with np.errstate(invalid="ignore"):
        guard = (x < 0) | (y < 0) | (z < 0)
    _, _, _, idx = oracle.select_project(x, y, z, None, 1.0, SLABS4[0], SLABS4[-1], BOX, 0, FOV, npix, want_index=True)
    sel = np.zeros(len(pos), bool)
    sel[idx] = True
    return np.where(guard, "G", np.where(sel, "S", "D"))


def table_outcome(c, setting, axis):
    return OUTCOMES[c].split()[setting][axis]


def pool(setting, kind):
    """The (class, axis) particles of a setting whose table outcome is in `kind` ("SD": quiet, "G": guard)."""
    labels, pos = class_particles(setting)
    keep = np.array([table_outcome(c, setting, a) in kind for c, a in labels])
    return [l for l, k in zip(labels, keep) if k], np.ascontiguousarray(pos[keep])


def interleave(ordinary, special, first=7):
    """`special` spread evenly through `ordinary` at fixed places, never at index 0 (the reference's guard is a
    min_element: a NaN as the FIRST element of an axis silences that axis, a quirk the device does not copy)."""
    n = len(ordinary) + len(special)
    at = first + (np.arange(len(special), dtype=np.int64) * (n - first - 1)) // max(len(special), 1)
    assert len(np.unique(at)) == len(special) and (len(at) == 0 or (at[0] > 0 and at[-1] < n))
    out = np.empty((n,) + ordinary.shape[1:], np.uint32)
    mask = np.zeros(n, bool)
    mask[at] = True
    out[mask] = np.ascontiguousarray(special).view(np.uint32)
    out[~mask] = np.ascontiguousarray(ordinary).view(np.uint32)
    return out.view(F32), at


def ordinary(n=20000):
    return synth.positions(0, n, BOX)
