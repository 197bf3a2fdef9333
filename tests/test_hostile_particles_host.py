"""What the reference path does with non-finite and out-of-domain particles, pinned without a GPU: the oracle
(oracle/slicer_oracle.c) and the second restatement (tests/np_restatement.py) agree bit for bit on every class of
tests/hostile_np.py, and each class's outcome equals the literal table there.  The device contract of
include/slicer_amd.h ("Hostile input") is stated against exactly these results; tests/test_gpu_hostile_particles.py holds
the device to them."""
import numpy as np
import pytest

import hostile_np as hn
import np_restatement as npr
import oracle
import tile_np as tnp

F32 = np.float32
QNAN = np.uint32(0x7FC00000)


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN (payloads are not part of the contract)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    ua, ub = np.where(np.isnan(a), QNAN, a.view(np.uint32)), np.where(np.isnan(b), QNAN, b.view(np.uint32))
    return a.shape == b.shape and np.array_equal(ua, ub)


def both_transforms(pos, setting):
    r = hn.SETTINGS[setting]
    a = oracle.transform(pos, hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    b = npr.transform(pos, hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    return a, b


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [512, 300, 64])
@pytest.mark.parametrize("setting", [0, 1])
def test_every_class_has_the_outcome_the_table_states(setting, npix):
    labels, pos = hn.class_particles(setting)
    assert set(hn.OUTCOMES) == set(hn.POSITION_CLASSES)
    assert hn.outcome(np.array([hn.BASES[setting]], F32), setting, npix)[0] == "S"  # "otherwise selected"
    got = hn.outcome(pos, setting, npix)
    want = np.array([hn.table_outcome(c, setting, a) for c, a in labels])
    bad = [(labels[i], got[i], want[i]) for i in np.nonzero(got != want)[0]]
    assert not bad, bad


@pytest.mark.parametrize("setting", [0, 1])
def test_pools_hold_what_the_gpu_tests_rely_on(setting):
    quiet, _ = hn.pool(setting, "SD")
    guard, _ = hn.pool(setting, "G")
    assert quiet and guard and len(quiet) + len(guard) == 3 * len(hn.POSITION_CLASSES)
    for c in ("qnan+", "qnan-", "qnan payload", "0x7F800001", "box+", "denormal min+", "denormal max-", "box 2^-100 -"):
        assert all((c, a) in quiet for a in range(3)), c
    # every role -- x, y, z -- meets a NaN, a guard class and a selected off-domain value in each setting
    assert {a for c, a in guard} == {0, 1, 2}
    selected = [(c, a) for c, a in quiet if hn.table_outcome(c, setting, a) == "S"]
    assert {a for c, a in selected if c in ("box+", "-0.0", "-0.1 box")} == {0, 1, 2}


def test_the_guard_is_per_particle_but_for_a_leading_nan():
    """any(x < 0 | y < 0 | z < 0) is what the reference's min_element guard computes -- unless a NaN leads an axis: NaN
    never loses a `<`, so min_element keeps it and the axis is silenced.  The device does not copy that (documented
    deviation); the GPU tests keep hostile values away from index 0."""
    setting = 0
    labels, pos = hn.class_particles(setting, ["-2.6 box", "qnan+"])
    bad = pos[labels.index(("-2.6 box", 1))]
    nan = pos[labels.index(("qnan+", 1))]  # raw axis 1 is x in setting 0, and -2.6 box makes x negative
    base = np.array(hn.BASES[setting], F32)
    for order, want in (([base, nan, bad], 1), ([base, bad, nan], 1), ([nan, base, bad], 0)):
        (x, y, z), _ = both_transforms(np.array(order, F32), setting)
        assert oracle.min_guard(x, y, z) == want, order
        with np.errstate(invalid="ignore"):
            assert bool(((x < 0) | (y < 0) | (z < 0)).any())


# ---- positions: oracle == restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [0, 1])
def test_positions_transform_selection_and_maps_agree(setting):
    labels, special = hn.class_particles(setting)  # every class, the guard ones too: the arithmetic is the same
    pos, at = hn.interleave(hn.ordinary(6000), special)
    (x, y, z), (x2, y2, z2) = both_transforms(pos, setting)
    assert same_bits(x, x2) and same_bits(y, y2) and same_bits(z, z2)
    assert np.isnan(np.stack([x, y, z])[:, at]).any() and np.isinf(np.stack([x, y, z])[:, at]).any()
    cls = {int(i): l for i, l in zip(at, labels)}
    for npix in (64, 300):
        chosen = set()
        for ld, ld2 in zip(hn.SLABS4[:-1], hn.SLABS4[1:]):
            xs, ys, ms, idx = oracle.select_project(x, y, z, None, 0.0123, ld, ld2, hn.BOX, 0, hn.FOV, npix, want_index=True)
            xs2, ys2, ms2, idx2 = npr.select_project(x, y, z, np.full(len(x), 0.0123, F32), ld, ld2, hn.BOX, 0, hn.FOV, npix)
            assert np.array_equal(idx, idx2) and len(idx) > 100
            assert np.array_equal(xs.view(np.uint32), xs2.view(np.uint32))
            assert np.array_equal(ys.view(np.uint32), ys2.view(np.uint32))
            # no selected entry has a non-finite map coordinate: the reference's (int)floor(x / dl) never sees one
            assert np.isfinite(xs).all() and np.isfinite(ys).all()
            assert np.abs(xs - 0.5).max() < 0.5 + 1.5 / npix and np.abs(ys - 0.5).max() < 0.5 + 1.5 / npix
            chosen |= set(int(i) for i in idx[np.isin(idx, at)])
            if npix == 64:
                for ngp in (False, True):
                    a, b = oracle.gridist_w(xs, ys, ms, npix, ngp), npr.gridist_w(xs, ys, ms, npix, ngp)
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all()
        for i, (c, a) in cls.items():  # (a guard class may be selected as well: the pass is aborted either way)
            assert (i in chosen) == {"S": True, "D": False}.get(hn.table_outcome(c, setting, a), i in chosen), (c, a)


# ---- masses: oracle == restatement, and where the NaNs are ------------------------------------------------------
def mass_case(setting, npix, n=6000):
    pos = hn.ordinary(n)
    r = hn.SETTINGS[setting]
    x, y, z = oracle.transform(pos, hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    _, _, _, idx = oracle.select_project(x, y, z, None, 1.0, hn.SLABS4[0], hn.SLABS4[-1], hn.BOX, 0, hn.FOV, npix,
                                         want_index=True)
    rng = np.random.default_rng(11 + setting)
    mass = ((1 + rng.permutation(n)).astype(np.float64) * 2.0 ** -20).astype(F32)
    names = list(hn.MASS_CLASSES)
    where = idx[1 + (np.arange(len(names)) * (len(idx) - 2)) // len(names)]  # selected particles, never the first one
    assert len(np.unique(where)) == len(names) and where.min() > 0
    mass.view(np.uint32)[where] = [hn.MASS_CLASSES[k] for k in names]
    return pos, mass, dict(zip(names, where))


@pytest.mark.parametrize("ngp", [False, True], ids=["tsc", "ngp"])
@pytest.mark.parametrize("setting", [0, 1])
def test_masses_maps_agree_and_the_nan_set_is_the_poisoned_footprints(setting, ngp):
    npix = 64
    pos, mass, where = mass_case(setting, npix)
    r = hn.SETTINGS[setting]
    f = dict(npart=[len(pos), 0, 0, 0, 0, 0], massarr=[0.0] * 6, boxsize=hn.BOX, pos=pos, mass={0: mass})
    rc, tot, toti, nsel = oracle.create_density_maps([f], 0, 1, npix, True, ngp, hn.SLABS4[0], hn.SLABS4[-1], 0, hn.FOV,
                                                     r["sgn"], r["face"], r["center"], r["rcase"])
    assert rc == 0
    x, y, z = npr.transform(pos, hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    xs, ys, ms, idx = npr.select_project(x, y, z, tnp.cap_mass(mass), hn.SLABS4[0], hn.SLABS4[-1], hn.BOX, 0, hn.FOV, npix)
    assert int(nsel[0]) == len(xs) and int(nsel.sum()) == len(xs)  # a poisoned particle is still a selected one
    ref = npr.gridist_w(xs, ys, ms, npix, ngp)
    assert same_bits(tot, ref) and same_bits(toti[0], ref)
    assert np.array_equal(np.isnan(tot), np.isnan(ref)) and np.array_equal(np.isinf(tot), np.isinf(ref))
    # where the NaNs (and NGP's infinities) are
    dl = 1.0 / np.float64(npix)
    gx = np.floor(xs.astype(np.float64) / dl).astype(np.int64)
    gy = np.floor(ys.astype(np.float64) / dl).astype(np.int64)
    want_nan, want_inf = np.zeros((npix, npix), bool), np.zeros((npix, npix), bool)
    for k, i in where.items():
        e = np.nonzero(idx == i)[0]
        assert len(e) == 1
        cx, cy = int(gx[e[0]]), int(gy[e[0]])
        if ngp:
            inside = 0 <= cx < npix and 0 <= cy < npix
            if inside and k in ("nan+", "nan-"):
                want_nan[cy, cx] = True
            if inside and k == "-inf":
                want_inf[cy, cx] = True
        elif hn.MASS_TSC[k] == "nan":
            for px in range(max(cx - 1, 0), min(cx + 2, npix)):  # the 3 x 3 footprint, clipped to the map: NaN * 0 is NaN
                for py in range(max(cy - 1, 0), min(cy + 2, npix)):
                    want_nan[py, px] = True
    assert want_nan.sum() >= (1 if ngp else 5 * 6)
    assert np.array_equal(np.isnan(tot), want_nan) and np.array_equal(np.isinf(tot), want_inf)
    if ngp:
        assert (tot[want_inf] < 0).all() and (tot[np.isfinite(tot)] < 0).sum() >= 1  # -inf; -1 and -2^-10 stay finite
    # the classes that add nothing but zero, and the ones that are kept: the map without them / with them as they are
    clean = mass.copy()
    for k, i in where.items():
        if hn.MASS_TSC[k] == "zero":
            clean[i] = 0.0
    _, tot2, _, nsel2 = oracle.create_density_maps([dict(f, mass={0: clean})], 0, 1, npix, True, ngp, hn.SLABS4[0],
                                                   hn.SLABS4[-1], 0, hn.FOV, r["sgn"], r["face"], r["center"], r["rcase"])
    assert same_bits(tot, tot2) and np.array_equal(nsel, nsel2)
    kept = ms[np.isin(idx, [where[k] for k in ("1000", "1000-", "denormal max", "FLT_MIN", "2^-100")])]
    assert len(kept) == 5 and (kept > 0).all() and kept.max() == F32(1000.0)  # m > MAX_M is false at 1000.0 exactly
