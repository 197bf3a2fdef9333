"""The deposit path on non-finite and out-of-domain particles (include/slicer_amd.h "Hostile input"), through
the C ABI.  Needs an MI355X.

The value classes and what the oracle does with each are tests/hostile_np.py (kept honest without a GPU by
tests/test_hostile_particles_host.py).  Everything expected comes from the oracle at test time; every pass asserts through
the algo mask which kernels ran.
  positions   quiet classes (the guard stays silent) among 20000 ordinary particles, on every route -- DIRECT, the fast
              project+bin kernel with and without wave stacks, the general one, the two-level sort: NGP maps and type maps
              bit for bit, FIXED64 TSC words exactly, nsel per plane and type.  Guard classes one at a time: every
              route reports SLICER_ERR_NEGATIVE_COORD exactly where the oracle returns 1.
  masses      NaN, negative and -inf per-particle masses poison their 3 x 3 footprint in the reference (sqrt -> NaN):
              F32 / F64 maps have exactly the oracle's NaN pixels and hold their bounds on all others (test_gpu_tile_deposit
              .check, E from the other entries); FIXED64 skips the entry and is exact; NGP maps are the oracle's bit for
              bit, NaN and -inf pixels included.  DIRECT and BINNED, integer and f64 tile cells.
  header      a constant mass that is NaN, negative or infinite is refused by slicer_file_begin.
"""
import functools

import numpy as np
import pytest

import hostile_np as hn
import k1_edges_np as ke
import oracle
import slicer_amd
import test_gpu_project_bin_fast as pbf
import test_gpu_tile_deposit as tdep

pytestmark = pytest.mark.gpu

F32 = np.float32
DIRECT, BINNED = slicer_amd.ALGO_DIRECT, slicer_amd.ALGO_BINNED
F32A, F64A, FIXA = slicer_amd.ACC_F32, slicer_amd.ACC_F64, slicer_amd.ACC_FIXED64
BATCH = 4096  # bin_batch: the 20000-odd particles of a pass fall into five workgroups of the project+bin kernel
OPTION_KEYS = tuple(sorted(set(pbf.OPTION_KEYS) | set(tdep.OPTION_KEYS)))
ROUTES = {"direct": dict(algo=DIRECT), "fast-stack0": dict(k1_stack=0), "fast-stack1": dict(k1_stack=1),
          "general": dict(k1_general=1), "sort2": dict(k1_stack=0, sort2=1)}


@pytest.fixture(scope="module")
def S0():
    s = slicer_amd.Slicer(0, max_chunk=1 << 20)
    yield s
    s.close()


@pytest.fixture
def S(S0):
    """The module's handle; every option a test sets is put back afterwards."""
    saved = {k: S0.get_option(k) for k in OPTION_KEYS}
    yield S0
    try:
        S0.set_option("k4_int", saved["k4_int"])
    except slicer_amd.api.SlicerError:  # a test that failed in mid-pass left deposits in flight: a new pass drops them
        S0.plane_begin(8, 1.0, [0.0], [1.0])
    for k, v in saved.items():
        S0.set_option(k, v)


def make_pass(setting, npix):
    return pbf.make_pass(npix, hn.FOV, hn.SETTINGS[setting], edges=hn.SLABS4, box=hn.BOX)


def run_route(S, ex, route, ngp):
    """One pass on a route; -> what pbf.check returns (the oracle's selected entries over the planes)."""
    opts = dict(ROUTES[route])
    algo = opts.pop("algo", BINNED)
    out, mask = pbf.run(S, ex, ngp=ngp, algo=algo, bin_batch=BATCH, **opts)
    sort2 = bool(opts.get("sort2")) and not ex.hydro
    if sort2 and ex.ps.npix == 512:  # (four planes of 512^2 qualify at this batch size; 300^2 may run either sort)
        assert mask & (1 << 7), f"{route}: the two-level sort did not run: mask {mask:#x}"
    return pbf.check(ex, out, mask, ngp=ngp, fast=route != "general", sort2=sort2 and bool(mask & (1 << 7)),
                     tag=f"{route} ngp={ngp}", algo=algo)


# ---- quiet positions --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def quiet_case(setting, npix):
    labels, special = hn.pool(setting, "SD")
    pos, at = hn.interleave(hn.ordinary(), special)
    assert at[0] > 0 and len(set(at // BATCH)) >= 4  # never first; the classes fall into several workgroups
    ex = pbf.Expect(make_pass(setting, npix), pos)
    chosen = np.concatenate([ex.index(p) for p in range(4)])
    for i, (c, a) in zip(at, labels):  # the oracle does with each class what the table says
        assert (i in chosen) == (hn.table_outcome(c, setting, a) == "S"), (c, a)
    return ex


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("npix", [512, 300])
@pytest.mark.parametrize("setting", [0, 1])
def test_quiet_positions_on_every_route(S, setting, npix, route):
    """Every quiet class on every raw axis (NaNs of either sign, with a payload, 0x7F800001; infinities and huge values
    on the axes where they do not trip the guard; box and beyond; -0.0; denormals; the kQLo end of the fast kernel's
    quotient range) among 20000 ordinary particles: the particle drops out or is selected exactly as in the oracle, no
    pixel and no counter differs."""
    ex = quiet_case(setting, npix)
    for ngp in (False, True):
        assert run_route(S, ex, route, ngp) > 3000


def quiet_nonfinite(g, n):
    """n raw positions with one coordinate NaN or infinite that leave the guard of geometry g silent."""
    base = pbf.clean_pool()[5000:5000 + 64].view(np.uint32)
    cand = []
    for c in ("qnan+", "qnan-", "qnan payload", "0x7F800001", "+inf", "-inf"):
        for a in range(3):
            p = base[len(cand) % len(base)].copy()
            p[a] = hn.POSITION_CLASSES[c]
            x, y, z = oracle.transform(p.view(F32)[None], g.box, g.sgn, g.face, g.center, g.rcase)
            with np.errstate(invalid="ignore"):
                if not ((x < 0) | (y < 0) | (z < 0)).any():
                    cand.append(p)
    assert len(cand) >= 12 + 3  # the NaNs on every axis, each infinity on at least one
    return np.array([cand[i % len(cand)] for i in range(n)], np.uint32).view(F32)


@pytest.mark.parametrize("n_bad", [255, 257])
def test_a_batch_full_of_nan_and_inf(S, n_bad):
    """One workgroup's batch (bin_batch = 4096) holds n_bad particles with a NaN or infinite coordinate and nothing else
    the fast kernel notes: 255 fit its exception list, 257 make it discard its records and redo the batch through
    process_exact.  The particles all drop out; maps, words and counts are the oracle's."""
    g = ke.Geometry.from_params(pbf.FIXTURE["a_params"])
    clean = pbf.clean_pool()
    batch = clean[:BATCH].copy()
    rng = np.random.default_rng(n_bad)
    at = np.sort(rng.choice(np.arange(1, BATCH), n_bad, replace=False))
    batch[at] = quiet_nonfinite(g, n_bad)
    pos = np.concatenate([clean[BATCH:2 * BATCH], batch, clean[2 * BATCH:3 * BATCH + 77]])
    noted = pbf.noted_by_kernel(pos, g)
    assert [int(noted[b:b + BATCH].sum()) for b in range(0, len(pos), BATCH)] == [0, n_bad, 0, 0]
    ex = pbf.Expect(pbf.make_pass(g.npix, g.fov, g.rnd, edges=g.edges), pos)
    chosen = np.concatenate([ex.index(p) for p in range(4)])
    assert not np.isin(BATCH + at, chosen).any() and len(chosen) > 1000
    for opts in (dict(k1_stack=0), dict(k1_stack=1), dict(k1_stack=0, sort2=1)):
        for ngp in (False, True):
            out, mask = pbf.run(S, ex, ngp=ngp, bin_batch=BATCH, **opts)
            assert bool(mask & (1 << 7)) == bool(opts.get("sort2")), f"two-level sort: mask {mask:#x}"
            pbf.check(ex, out, mask, ngp=ngp, sort2=bool(opts.get("sort2")), tag=f"{n_bad} non-finite {opts} ngp={ngp}")


# ---- guard positions --------------------------------------------------------------------------------------------
def oracle_rc(pos, setting, npix):
    r = hn.SETTINGS[setting]
    f = dict(npart=[0, len(pos), 0, 0, 0, 0], massarr=[0, pbf.M_CONST, 0, 0, 0, 0], boxsize=hn.BOX, pos=pos)
    return oracle.create_density_maps([f], 0, 1, npix, False, True, hn.SLABS4[0], hn.SLABS4[-1], 0, hn.FOV, r["sgn"],
                                      r["face"], r["center"], r["rcase"])[0]


def expect_guard(S, pos, setting, route, npix=512, ngp=True):
    assert oracle_rc(pos, setting, npix) == 1
    opts = dict(ROUTES[route])
    algo = opts.pop("algo", BINNED)
    ex = pbf.Expect(make_pass(setting, npix), pos)
    with pytest.raises(slicer_amd.SlicerError) as err:
        pbf.run(S, ex, ngp=ngp, algo=algo, bin_batch=BATCH, **opts)
    assert err.value.code == slicer_amd.api.ERR_NEGATIVE_COORD
    mask = S.algo_mask()
    if algo == DIRECT:
        assert (mask & 7) == 1 << DIRECT
    else:
        want = pbf.GENERAL if route == "general" else pbf.FAST
        assert (mask & 7) == 1 << BINNED and (mask & (pbf.FAST | pbf.GENERAL)) == want, f"mask {mask:#x}"


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("setting", [0, 1])
def test_every_guard_class_alone_trips_the_guard(S, setting, route):
    """Each guard class (infinities and huge values whose sign after the axis' mirror is negative, 2 box, 2.5 box,
    -2.6 box) as the only hostile particle of a pass: the oracle returns 1, plane_read raises code 1."""
    labels, special = hn.pool(setting, "G")
    ordinary = hn.ordinary()
    assert oracle_rc(ordinary, setting, 512) == 0
    assert len(labels) >= 10
    for k, (c, a) in enumerate(labels):
        pos, at = hn.interleave(ordinary, special[k:k + 1], first=1 + 997 * k)  # (moves through the workgroups)
        expect_guard(S, pos, setting, route, ngp=bool(k & 1))


@pytest.mark.parametrize("route", list(ROUTES))
def test_a_guard_class_and_a_nan_together(S, route):
    """A NaN on the same transformed axis, before and after the guard particle (never first), does not hide it."""
    setting = 0
    labels, special = hn.class_particles(setting, ["qnan+", "-2.6 box", "qnan-"])
    pick = np.array([special[labels.index((c, 1))] for c in ("qnan+", "-2.6 box", "qnan-")], F32)
    pos, at = hn.interleave(hn.ordinary(), pick, first=4097)
    for npix in (512, 300):
        expect_guard(S, pos, setting, route, npix=npix, ngp=npix == 300)


# ---- masses -----------------------------------------------------------------------------------------------------
def exact_masses(n, seed):
    return pbf.exact_masses(n, np.random.default_rng(seed))


@functools.lru_cache(maxsize=4)
def ngp_mass_case(setting, npix):
    """Every mass class on a selected particle of each plane, the others with exact_masses (any sum of a pixel's masses
    is exact: NGP maps do not depend on the order of the additions, so the oracle's map is the expected one bit for
    bit)."""
    pos = hn.ordinary()
    mass = exact_masses(len(pos), 40 + setting)
    plain = pbf.Expect(make_pass(setting, npix), pos)
    names = list(hn.MASS_CLASSES)
    for p in range(4):
        idx = plain.index(p)
        where = idx[3 + (np.arange(len(names)) * (len(idx) - 4)) // len(names)]
        assert len(np.unique(where)) == len(names) and where.min() > 0
        mass.view(np.uint32)[where] = [hn.MASS_CLASSES[k] for k in names]
    ex = pbf.Expect(make_pass(setting, npix), pos, mass)
    nan = sum(int(np.isnan(ex.ngp(p)[0]).sum()) for p in range(4))
    neg_inf = sum(int(np.isneginf(ex.ngp(p)[0]).sum()) for p in range(4))
    assert nan >= 4 and neg_inf >= 2 and not any(np.isposinf(ex.ngp(p)[0]).any() for p in range(4)), (nan, neg_inf)
    return ex


@pytest.mark.parametrize("route", ["direct", "fast-stack0", "fast-stack1", "general"])
@pytest.mark.parametrize("npix", [512, 300])
@pytest.mark.parametrize("setting", [0, 1])
def test_mass_classes_ngp_and_fixed64(S, setting, npix, route):
    """NGP with masses: the oracle's maps bit for bit -- a NaN mass gives a NaN pixel, -inf a -inf pixel, -1 a finite
    negative one, masses above MAX_M (+inf, FLT_MAX, nextafter(1000)) nothing, 1000.0 exactly is kept.  TSC in FIXED64:
    the entries whose root is NaN add nothing, the words are exact over the others, the map is finite, nsel counts
    every selected entry."""
    ex = ngp_mass_case(setting, npix)
    for ngp in (True, False):
        assert run_route(S, ex, route, ngp) > 3000


# (TSC with masses in F32 / F64 / FIXED64: test_gpu_tile_deposit's Case -- one plane over the four slabs' range, 64 x 64
# tiles forced, so that J of its bounds is known)
TL = 6
POISON = hn.POISON_MASSES  # nan+, nan-, -1, -2^-10, -inf
BENIGN = [k for k in hn.MASS_CLASSES if k not in POISON and k not in ("1000", "1000-")]  # (those set the quantum: below)


def tsc_modes(S, case, tag, int_cells_too=True):
    """BINNED: F32, F64, FIXED64 with integer (k4_int = 2) and f64 (0) tile cells; DIRECT: the three accumulators."""
    S.set_option("bin_batch", BATCH)
    S.set_option("k1_stack", -1)
    for accum in (F32A, F64A, FIXA):
        for k4 in (2, 0):
            tot, acc, mask = tdep.run(S, case, accum, k4)
            tdep.check(case, tot, acc, mask, accum, k4, tag=f"{tag} binned {tdep.ACC_IDS[accum]} k4_int={k4}")
        tot, acc, mask = tdep.run(S, case, accum, 0, algo=DIRECT)
        tdep.check(case, tot, acc, mask, accum, 0, tag=f"{tag} direct {tdep.ACC_IDS[accum]}", algo=DIRECT)


def poisoned_pixels(case):
    """The union of the poisoned entries' 3 x 3 footprints, clipped to the map (what the host test proves the oracle's
    NaN set to be)."""
    want = np.zeros((case.npix, case.npix), bool)
    for cx, cy in zip(case.gx[case.poisoned], case.gy[case.poisoned]):
        want[max(cy - 1, 0):min(cy + 2, case.npix), max(cx - 1, 0):min(cx + 2, case.npix)] = True
    return want


@functools.lru_cache(maxsize=2)
def placed_case(npix):
    """20000 ordinary particles with exact_masses and the benign classes, plus poisoned particles placed inside a tile,
    on a tile seam (footprint over 2 and over 4 bins), in the map's first column (footprint clipped), in the border ring
    (centre off the map), and two in one pixel -- one of each per poisoned class."""
    rng = np.random.default_rng(50 + npix)
    spots, masses = [], []
    for j, k in enumerate(POISON):
        o = 6 * j
        corner = [(63, 63), (127, 63), (191, 63), (255, 63), (63, 127)][j]  # four tiles meet at its upper right
        rects = [(80 + o, 90), (63, 70 + o), corner, (0, 100 + o), (-1, 140 + o), (150 + o, 160), (150 + o, 160)]
        for px, py in rects:
            spots.append(tdep.place(1, npix, (px + 0.1, px + 0.9, py + 0.1, py + 0.9), rng))
            masses.append(hn.MASS_CLASSES[k])
    ordinary = hn.ordinary()
    mass = exact_masses(len(ordinary), 60)
    selected = tdep.forward(ordinary, None, 1.0, npix)[3]
    where = selected[5 + (np.arange(len(BENIGN)) * (len(selected) - 6)) // len(BENIGN)]
    mass.view(np.uint32)[where] = [hn.MASS_CLASSES[k] for k in BENIGN]
    pos, at = hn.interleave(ordinary, np.concatenate(spots))
    m, _ = hn.interleave(mass, np.array(masses, np.uint32).view(F32))
    case = tdep.Case(npix, TL, pos, m, tdep.M_CONST)
    assert int(case.poisoned.sum()) == len(spots) and np.array_equal(np.sort(case.idx[case.poisoned]), at)
    assert np.array_equal(case.nan_mask, poisoned_pixels(case))
    gx, gy = case.gx[case.poisoned], case.gy[case.poisoned]
    assert (gx == -1).sum() == len(POISON) and (gx == 0).sum() == len(POISON)                 # ring; clipped
    assert ((gx == 63) & (gy % 64 != 63)).sum() == len(POISON) and ((gx % 64 == 63) & (gy % 64 == 63)).sum() == len(POISON)  # seams
    assert 9 * 3 * len(POISON) < case.nan_mask.sum() < 9 * len(spots)
    assert case.le <= -4 and np.isin(hn.mass_values(["denormal min", "denormal max", "FLT_MIN", "2^-100"]), case.ms).all()
    return case


@pytest.mark.parametrize("npix", [512, 300])
def test_poisoned_masses_tsc_placed(S, npix):
    """The NaN pixels of F32 / F64 maps are exactly the oracle's -- the poisoned 3 x 3 footprints, also where one spans
    two or four tiles or is clipped by the map's edge -- and every other pixel holds its bound; FIXED64 is exact over
    the other entries and finite."""
    tsc_modes(S, placed_case(npix), f"placed npix={npix}")


NPIX = tdep.NPIX  # 256: 4 x 4 tiles of 64 x 64 pixels


@functools.lru_cache(maxsize=1)
def many_poisoned_case():
    rng = np.random.default_rng(70)
    normal = tdep.place(6000, NPIX, (64 + 2.05, 64 + 29.95, 64 + 2.05, 64 + 49.95), rng)
    bad = tdep.place(600, NPIX, (64 + 34.1, 64 + 59.9, 64 + 2.1, 64 + 49.9), rng)
    mass = np.r_[rng.uniform(1.0e-5, 1.9e-5, 6000).astype(F32), hn.mass_values([POISON[i % len(POISON)] for i in range(600)])]
    return tdep.Case(NPIX, TL, np.concatenate([normal, bad]), mass.astype(F32), tdep.M_CONST)


def test_more_poisoned_records_than_the_noted_list_holds(S):
    """600 poisoned records in one work item: 512 wait in the LDS list of noted records, the others go through the
    inline slow_record."""
    case = many_poisoned_case()
    assert case.bin_count(tdep.INTERIOR) == len(case.xs) == 6600 <= 32768 and int(case.poisoned.sum()) == 600 > 512
    assert np.array_equal(case.nan_mask, poisoned_pixels(case))
    tsc_modes(S, case, "600 poisoned")


@functools.lru_cache(maxsize=1)
def split_bin_case():
    rng = np.random.default_rng(71)
    pos = tdep.place(40000, NPIX, (64 + 0.05, 64 + 63.95, 64 + 0.05, 64 + 63.95), rng)
    mass = tdep.decade_masses(len(pos), rng)
    mass[23456] = hn.mass_values(["nan+"])[0]
    return tdep.Case(NPIX, TL, pos, mass, tdep.M_CONST)


def test_one_poisoned_record_in_a_split_bin(S):
    """40000 records in one bin -- three parts under integer cells (above kWholeRecsInt = 32768), whole otherwise -- and
    one NaN mass among them."""
    case = split_bin_case()
    assert case.bin_count(tdep.INTERIOR) == 40000 and int(case.poisoned.sum()) == 1
    assert int(tdep.tnp.parts_of(40000, True)) == 3 and int(tdep.tnp.parts_of(40000, False)) == 1
    assert case.nan_mask.sum() == 9
    tsc_modes(S, case, "split bin")


@functools.lru_cache(maxsize=1)
def heavy_bin_case():
    rng = np.random.default_rng(73)
    px, py = 64 + 5, 64 + 7
    pos = tdep.place(114689, NPIX, (px + 0.02, px + 0.98, py + 0.02, py + 0.98), rng)
    mass = tdep.decade_masses(len(pos), rng)
    mass.view(np.uint32)[[777, 100001]] = [hn.MASS_CLASSES["nan-"], hn.MASS_CLASSES["-1"]]
    return tdep.Case(NPIX, TL, pos, mass, tdep.M_CONST)


def test_poisoned_records_in_a_heavy_bin(S):
    """114689 records in one pixel -- eight parts, the fewest that take the heavy-bin walk with its wave-level
    pre-reduction (merged_run) -- two of them poisoned: the footprint is NaN in F32 / F64, FIXED64 sums the others."""
    case = heavy_bin_case()
    assert case.bin_count(tdep.INTERIOR) == 114689 and int(tdep.tnp.parts_of(114689, False)) == 8
    assert int(case.poisoned.sum()) == 2 and case.nan_mask.sum() == 9
    tsc_modes(S, case, "heavy bin")


@functools.lru_cache(maxsize=4)
def quantum_case(big):
    rng = np.random.default_rng(72)
    pos = tdep.place(3000, NPIX, (64 + 2.05, 3 * 64 - 2.05, 64 + 2.05, 3 * 64 - 2.05), rng)
    mass = np.full(len(pos), 2.0 ** -20, F32)
    mass.view(np.uint32)[1500] = big
    return tdep.Case(NPIX, TL, pos, mass, tdep.M_CONST)


@pytest.mark.parametrize("big,le", [(hn.bits_of(-1000.0), -19), (hn.MASS_CLASSES["nan+"], -19), (hn.MASS_CLASSES["1000"], 10),
                                    (hn.MASS_CLASSES["1000+"], -19)], ids=["-1000", "nan", "1000", "1000+"])
def test_the_quantum_comes_from_the_finite_masses(S, big, le):
    """Every mass is 2^-20 but one.  -1000 or NaN: the integer cells' quantum must come from the finite masses
    (2^le = 2^-19 above them), or every ordinary contribution would miss the cells' grid; the poisoned footprint is NaN.
    1000.0 exactly is kept (m > MAX_M is false) and sets 2^le = 2^10; the next f32 above counts as 0."""
    case = quantum_case(big)
    assert case.le == le and len(case.xs) == 3000
    assert (case.nan_mask is not None) == (le == -19 and big != hn.MASS_CLASSES["1000+"])
    if big == hn.MASS_CLASSES["1000"]:
        assert case.ms.max() == F32(1000.0)
    tsc_modes(S, case, f"quantum le={le}")


# ---- header masses ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, -1.0, np.inf, -np.inf])
def test_a_corrupt_header_mass_is_refused(S, value):
    S.plane_begin(64, hn.FOV, [3.0], [4.0], algo=BINNED)
    r = hn.SETTINGS[0]
    with pytest.raises(slicer_amd.SlicerError) as err:
        S.file_begin([0, 5, 0, 0, 0, 0], [0.0, value, 0.0, 0.0, 0.0, 0.0], hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    assert err.value.code == 2  # SLICER_ERR_ARG
    text = str(err.value).lower()
    assert "massarr[1]" in text and ("nan" in text if np.isnan(value) else ("inf" in text if np.isinf(value) else "-1" in text))
    # a type without particles is not looked at, and the handle takes the next file
    S.file_begin([0, 5, 0, 0, 0, 0], [value, 0.5, 0.0, 0.0, 0.0, 0.0], hn.BOX, r["sgn"], r["face"], r["center"], r["rcase"])
    S.file_end()


@pytest.mark.parametrize("route", ["direct", "fast-stack0", "general"])
def test_a_header_mass_above_max_m_is_deposited_as_is(S, route):
    """The cap at MAX_M applies to per-particle masses only (densitymaps.cpp:367-369): massarr = 2000 is deposited."""
    ex = pbf.Expect(make_pass(0, 300), hn.ordinary(), mconst=2000.0)
    assert float(ex.ngp(0)[0].max()) >= 2000.0
    for ngp in (True, False):
        assert run_route(S, ex, route, ngp) > 3000
