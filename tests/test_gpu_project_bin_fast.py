"""The fast project+bin kernel (k_project_bin_fast) bit for bit against the oracle, through the C ABI.  Needs an MI355X.

Expected values always come from the oracle at test time (oracle.transform + oracle.select_project, and
oracle.create_density_maps for NGP), never from the device or a recorded output.  Every pass asks for ALGO_BINNED and
asserts which project+bin kernel ran (slicer_plane_algo_mask: bit 4 the fast kernel, bit 5 the general one).  Three
observables, all compared exactly:
  TSC, FIXED64   accumulator words == sum rint(c 2^e) over the oracle's (xs, ys, m) (tests/tile_np.py, asserted by
                 test_gpu_tile_deposit.check): one wrong bit of xs, ys, the plane or the selection changes a word;
  NGP            maps and per-type maps == the oracle's;
  nsel           per-type selected counts == the oracle's.
tests/golden/k1_edges.npz holds raw positions at the kernel's decision edges (tests/k1_edges_np.py has the classes,
tests/test_k1_edges_host.py keeps the file honest).
Expect, run and check also serve tests/test_gpu_hostile_particles.py, which runs the same passes through ALGO_DIRECT as
well and feeds per-particle masses that are NaN or negative (check compares NGP maps with the oracle's NaN pixels).
"""
import functools
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import k1_edges_np as ke
import np_restatement as npr
import oracle
import slicer_amd
import test_gpu_tile_deposit as tdep
import tile_np as tnp
from slicer_amd import synth

pytestmark = pytest.mark.gpu

BOX = 1000.0
F32C = tuple(float(np.float32(c)) for c in (0.3, 0.6, 0.1))  # binary32 centres >= 2^-20: the fast kernel qualifies
FIXA, F32A = slicer_amd.ACC_FIXED64, slicer_amd.ACC_F32
M_CONST = 0.0123
SLABS4 = [3.0, 3.25, 3.5, 3.75, 4.0]  # four consecutive slabs of one box replication (rcase 3)
FAST, GENERAL = 1 << 4, 1 << 5
OPTION_KEYS = ("k4_int", "tile_log2", "tile_h_log2", "bin_batch", "unit_rows", "k1_general", "k1_stack", "sort2", "pending",
               "k3_per_cu")
GEOMETRY_KEYS = ("tile_log2", "tile_h_log2", "pending", "k3_per_cu")  # run() sets these only where a caller names them
SERIES_MAX9 = 0.155  # slicer_device.hpp: kSeriesMax9 (fov 0.25 runs the 9-term series)


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


# ---- the pass, its expected values, the comparison ------------------------------------------------------------------
def make_pass(npix, fov, rnd, edges=SLABS4, box=BOX, slabs=None, nrep=0):
    slabs = slabs if slabs is not None else list(zip(edges[:-1], edges[1:]))
    return SimpleNamespace(npix=npix, fov=fov, rnd=rnd, box=box, slabs=slabs, nrep=nrep)


def rnd_of(face, sgn, center=F32C, rcase=3.0):
    return dict(sgn=tuple(sgn), face=face, center=tuple(center), rcase=rcase)


class Expect:
    """The oracle's entries of every plane of the pass for one species (constant mass or per-particle masses)."""

    def __init__(self, ps, pos, mass=None, mconst=M_CONST):
        self.ps, self.pos, self.mass, self.mconst = ps, np.ascontiguousarray(pos, np.float32), mass, mconst
        self.hydro = mass is not None
        self.ptype = 0 if self.hydro else 1
        r = ps.rnd
        x, y, z = oracle.transform(self.pos, ps.box, r["sgn"], r["face"], r["center"], r["rcase"])
        self._tsc, self._ngp = {}, {}
        self.entries = [oracle.select_project(x, y, z, mass, 0.0 if self.hydro else mconst, ld, ld2, ps.box, ps.nrep,
                                              ps.fov, ps.npix, want_index=True) for ld, ld2 in ps.slabs]

    def index(self, p):
        return self.entries[p][3]

    def tsc(self, p):
        """What test_gpu_tile_deposit.check compares a FIXED64 plane with."""
        if p not in self._tsc:
            self._tsc[p] = self._make_tsc(p)
        return self._tsc[p]

    def _make_tsc(self, p):
        xs, ys, ms, _ = self.entries[p]
        # (the cap at MAX_M is for per-particle masses only: densitymaps.cpp:367-369; a NaN or negative one poisons its
        # footprint in the reference, and the FIXED64 accumulator skips the entry)
        ms, _ = tdep.clean_mass(tnp.cap_mass(ms) if self.hydro else ms)
        pix, val = npr.tsc_contributions(xs, ys, ms, self.ps.npix)
        le = tnp.mass_le(ms.max(initial=0.0) if self.hydro else self.mconst)
        return SimpleNamespace(P=tnp.Pixels(pix, val, self.ps.npix, le), E=None, k=None, npix=self.ps.npix,
                               fixed_exp=40 - (10 if self.hydro else tnp.mass_le(self.mconst)), n=len(xs))

    def ngp(self, p):
        if p not in self._ngp:
            self._ngp[p] = self._make_ngp(p)
        return self._ngp[p]

    def _make_ngp(self, p):
        ps, r, n = self.ps, self.ps.rnd, len(self.pos)
        npart, massarr = [0] * 6, [0.0] * 6
        npart[self.ptype], massarr[self.ptype] = n, 0.0 if self.hydro else self.mconst
        f = dict(npart=npart, massarr=massarr, boxsize=ps.box, pos=self.pos, mass={0: self.mass} if self.hydro else {})
        rc, tot, toti, nsel = oracle.create_density_maps([f], 0, 1, ps.npix, self.hydro, True, ps.slabs[p][0],
                                                         ps.slabs[p][1], ps.nrep, ps.fov, r["sgn"], r["face"], r["center"],
                                                         r["rcase"])
        assert rc == 0
        return tot, toti, nsel


def run(S, ex, ngp, chunks=None, deposit=None, algo=slicer_amd.ALGO_BINNED, **options):
    """One pass over ex.pos as one file (deposit calls `chunks`, default one); -> per plane (tot, toti, nsel, acc), mask."""
    ps, r, n = ex.ps, ex.ps.rnd, len(ex.pos)
    for k in ("k1_general", "k1_stack", "sort2", "unit_rows", "bin_batch"):
        S.set_option(k, options.get(k, {"k1_stack": -1}.get(k, 0)))
    for k in GEOMETRY_KEYS:  # (tests/test_gpu_sort.py forces the whole geometry; the S fixture puts the values back)
        if k in options:
            S.set_option(k, options[k])
    assert not set(options) - set(OPTION_KEYS), set(options) - set(OPTION_KEYS)
    S.plane_begin(ps.npix, ps.fov, [a for a, _ in ps.slabs], [b for _, b in ps.slabs], [ps.nrep] * len(ps.slabs),
                  mas=slicer_amd.MAS_NGP if ngp else slicer_amd.MAS_TSC, accum=F32A if ngp else FIXA,
                  algo=algo, hydro=ex.hydro)
    npart, massarr = [0] * 6, [0.0] * 6
    npart[ex.ptype], massarr[ex.ptype] = n, 0.0 if ex.hydro else ex.mconst
    S.file_begin(npart, massarr, ps.box, r["sgn"], r["face"], r["center"], r["rcase"])
    if deposit is not None:
        deposit(S, ex)
    else:
        for a, b in chunks or [(0, n)]:
            S.deposit_host(ex.ptype, ex.pos[a:b], ex.mass[a:b] if ex.hydro else None)
    S.file_end()
    accs = [None] * len(ps.slabs)
    if not ngp:
        S.plane_flush()
        for p in range(len(ps.slabs)):
            ptrs, _ = S.plane_accumulators(p)
            accs[p] = S.to_host(ptrs[ex.ptype], (ps.npix, ps.npix), np.uint64)
    out = [S.plane_read(p) + (accs[p],) for p in range(len(ps.slabs))]
    return out, S.algo_mask()


def check(ex, out, mask, ngp, fast=True, sort2=False, tag="", algo=slicer_amd.ALGO_BINNED):
    """NGP maps are compared bit for bit, any NaN of the oracle's matching any NaN here (tdep.same_bits: a pixel that is
    NaN on one side only differs)."""
    if algo == slicer_amd.ALGO_DIRECT:
        assert (mask & 7) == 1 << slicer_amd.ALGO_DIRECT and not mask & (FAST | GENERAL), f"{tag}: DIRECT did not run alone: mask {mask:#x}"
    else:
        assert (mask & 7) == 1 << slicer_amd.ALGO_BINNED, f"{tag}: the binned path did not run alone: mask {mask:#x}"
        if fast:
            assert mask & FAST and not mask & GENERAL, f"{tag}: the fast kernel did not run alone: mask {mask:#x}"
        else:
            assert mask & GENERAL and not mask & FAST, f"{tag}: the pass was not refused: mask {mask:#x}"
    total = 0
    for p, (tot, toti, nsel, acc) in enumerate(out):
        t = f"{tag} plane {p}"
        if ngp:
            ref_tot, ref_toti, ref_nsel = ex.ngp(p)
            assert np.array_equal(nsel, ref_nsel), f"{t}: nsel {nsel} != {ref_nsel}"
            assert tdep.same_bits(tot, ref_tot), f"{t}: NGP map differs"
            assert tdep.same_bits(toti, ref_toti), f"{t}: NGP type maps differ"
            total += int(ref_nsel.sum())
        else:
            case = ex.tsc(p)
            assert int(nsel[ex.ptype]) == case.n and int(nsel.sum()) == case.n, f"{t}: nsel {nsel} != {case.n}"
            assert np.array_equal(tot.view(np.uint32), toti[ex.ptype].view(np.uint32)), t
            tdep.check(case, tot, acc, mask, FIXA, 0, int(sort2), tag=t, algo=algo)
            total += case.n
    return total


def edge_product():
    vals = np.array([0.0, -0.0, BOX, 1e-30, 0.5 * BOX, 0.999999 * BOX, np.nextafter(np.float32(BOX), np.float32(0))],
                    np.float32)
    return np.array(list(itertools.product(vals, repeat=3)), np.float32)


@functools.lru_cache(maxsize=None)
def matrix_positions():
    return np.concatenate([synth.positions(0, 40000, BOX), edge_product()])


def exact_masses(n, rng):
    """A distinct mass per particle, every one a multiple of 2^-20 below 2^-4 (any sum of a pixel's masses is exact in
    f32, so NGP maps do not depend on the order of the additions); ~1 % are 0 and ~1 % above MAX_M (they count as 0)."""
    m = ((1 + rng.permutation(n)).astype(np.float64) * 2.0 ** -20).astype(np.float32)
    assert n < 1 << 16
    m[rng.random(n) < 0.01] = 0.0
    m[rng.random(n) < 0.01] = 2000.0
    return m


# ---- A. the transform and emission matrix -----------------------------------------------------------------------
@pytest.mark.parametrize("fov", [0.25, 0.5], ids=["series9", "series15"])
@pytest.mark.parametrize("npix", [512, 300])
@pytest.mark.parametrize("face", [1, 2, 3, 4, 5, 6])
def test_transform_matrix_fixed64(S, face, npix, fov):
    """All 8 sign triples of a face, with and without the wave stacks, four planes in one pass: TSC, constant mass,
    FIXED64.  fov 0.25 runs the 9-term series, 0.5 the 15-term one (k1_fast_args: k_dec * 1.001 + 1e-4 against
    kSeriesMax9 = 0.155 -- 0.127 and 0.265); 512 / 300 are the POW2 instantiations."""
    pos = matrix_positions()
    for sgn in itertools.product((-1, 1), repeat=3):
        ex = Expect(make_pass(npix, fov, rnd_of(face, sgn)), pos)
        for stack in (0, 1):
            out, mask = run(S, ex, ngp=False, k1_stack=stack)
            assert check(ex, out, mask, ngp=False, tag=f"face {face} sgn {sgn} stack {stack}") > 15000


MODE_SIGNS = {1: (1, 1, 1), 2: (-1, 1, 1), 3: (-1, 1, -1), 4: (1, -1, -1), 5: (1, -1, 1), 6: (-1, -1, -1)}


@pytest.mark.parametrize("npix", [512, 300])
@pytest.mark.parametrize("face", [1, 2, 3, 4, 5, 6])
def test_emission_modes(S, face, npix):
    """The emission instantiations: NGP (kEmitLeanNgp), TSC with per-particle masses (kEmitLeanMass), NGP with masses
    and band units (kEmitGeneric), the two-level sort (kEmitSort2).  Every particle carries its own mass: a record that
    fetched another particle's mass shows in the accumulator."""
    pos = matrix_positions()
    ps = make_pass(npix, 0.25, rnd_of(face, MODE_SIGNS[face]))
    const = Expect(ps, pos)
    hydro = Expect(ps, pos, exact_masses(len(pos), np.random.default_rng(face)))
    assert len(np.unique(hydro.mass)) > 0.97 * len(pos)
    for stack in (0, 1):
        for ex, ngp, opts, name in ((const, True, {}, "ngp"), (hydro, False, {}, "tsc+mass"), (hydro, True, {}, "ngp+mass"),
                                    (const, False, dict(unit_rows=3), "bands"), (const, True, dict(unit_rows=3), "bands ngp")):
            out, mask = run(S, ex, ngp=ngp, k1_stack=stack, **opts)
            check(ex, out, mask, ngp=ngp, tag=f"face {face} {name} stack {stack}")


@pytest.mark.parametrize("npix", [512, 300])
@pytest.mark.parametrize("face", [1, 2, 3, 4, 5, 6])
def test_emission_two_level_sort(S, face, npix):
    ex = Expect(make_pass(npix, 0.25, rnd_of(face, MODE_SIGNS[face])), matrix_positions())
    out, mask = run(S, ex, ngp=False, k1_stack=0, sort2=1)
    if not mask & (1 << 7):
        pytest.skip("the pass does not qualify for the two-level sort")
    check(ex, out, mask, ngp=False, sort2=True, tag=f"face {face} sort2")
    out, mask = run(S, ex, ngp=True, k1_stack=0, sort2=1)
    check(ex, out, mask, ngp=True, tag=f"face {face} sort2 ngp")


REFUSALS = {
    "double_centre": dict(rnd=rnd_of(3, (-1, 1, -1), center=(0.3, 0.6, 0.1))),
    "tiny_centre": dict(rnd=rnd_of(3, (-1, 1, -1), center=(F32C[0], 2.0 ** -21, F32C[2]))),
    "five_planes": dict(edges=[3.0, 3.2, 3.4, 3.6, 3.8, 4.0]),
    "nrep1": dict(nrep=1),
    "gaps": dict(slabs=[(3.0, 3.2), (3.3, 3.5), (3.6, 3.8), (3.9, 4.0)]),
    "box0.1": dict(box=0.1, edges=[e * 1e-4 for e in SLABS4]),
}


@pytest.mark.parametrize("why", list(REFUSALS))
def test_refused_passes_run_the_general_kernel_and_stay_exact(S, why):
    kw = dict(REFUSALS[why])
    rnd = kw.pop("rnd", rnd_of(3, (-1, 1, -1)))
    ps = make_pass(512, 0.25, rnd, **kw)
    pos = matrix_positions() if ps.box == BOX else (matrix_positions() * np.float32(1e-4)).astype(np.float32)
    ex = Expect(ps, pos)
    for ngp in (False, True):
        out, mask = run(S, ex, ngp=ngp)
        assert check(ex, out, mask, ngp=ngp, fast=False, tag=why) > 15000


# ---- B. mined decision edges --------------------------------------------------------------------------------------
FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "k1_edges.npz"))


@functools.lru_cache(maxsize=None)
def edge_case(name):
    g = ke.Geometry.from_params(FIXTURE[name + "_params"])
    special = FIXTURE[name + "_pos"]
    rng = np.random.default_rng(7)
    n = len(special) + 20000
    at = np.sort(rng.choice(n, len(special), replace=False))  # the classes interleaved with ordinary particles
    pos = np.empty((n, 3), np.float32)
    mask = np.zeros(n, bool)
    mask[at] = True
    pos[mask], pos[~mask] = special, synth.positions(0, 20000, g.box)
    return g, pos, at, FIXTURE[name + "_label"]


@pytest.mark.parametrize("name", ["a", "b", "c"], ids=["512", "300", "300-fov0.5"])
def test_mined_decision_edges(S, name):
    """Ties, border rings, the FOV limit, the pre-test's margin, slab thresholds and cell boundaries (k1_edges.npz)
    as one file among 20000 ordinary particles: FIXED64 and NGP, both stack settings, and the general kernel on the
    same input (a difference between oracle and device is then the fast kernel's or not)."""
    g, pos, at, lab = edge_case(name)
    ex = Expect(make_pass(g.npix, g.fov, g.rnd, edges=g.edges), pos)
    # the decisions the classes stand for are real ones: across every slab threshold and FOV limit the oracle's
    # selected set differs
    e = ke.Entries(pos[at], g)
    planes = np.zeros(len(pos), np.int64) - 1
    for p in range(4):
        planes[ex.index(p)] = p
    assert np.array_equal(planes[at], np.where(e.selected, e.plane, -1))
    zed = ke.z_edge(e.z, g)
    on_z = (lab & ke.Z) != 0
    for k in range(5 if name != "c" else 0):
        assert np.all(planes[at][on_z & (zed == 2 * k)] == (k if k < 4 else -1)) and (on_z & (zed == 2 * k)).sum() >= 4
        assert np.all(planes[at][on_z & (zed == 2 * k + 1)] == k - 1) and (on_z & (zed == 2 * k + 1)).sum() >= 4
    for inside, outside in ((ke.F_DEC_IN, ke.F_DEC_OUT), (ke.F_RA_IN, ke.F_RA_OUT)):
        assert np.all(planes[at][(lab & inside) != 0] >= 0) and np.all(planes[at][(lab & outside) != 0] == -1)
        assert ((lab & inside) != 0).sum() >= 8 and ((lab & outside) != 0).sum() >= 8
    for opts, fast in ((dict(k1_stack=0), True), (dict(k1_stack=1), True), (dict(k1_general=1), False)):
        for ngp in (False, True):
            out, mask = run(S, ex, ngp=ngp, **opts)
            check(ex, out, mask, ngp=ngp, fast=fast, tag=f"{name} {opts} ngp={ngp}")


# ---- C. the exception list at its edges ---------------------------------------------------------------------------
BATCH = 4096  # bin_batch of the tests below: one workgroup reads particles [4096 w, 4096 (w + 1))


def off_domain(n, rng):
    """n particles the domain test notes (-0.0, beyond the box, negative: |excess| < 0.3 box keeps every transformed
    coordinate in [0, 1], so the negativity guard stays quiet), as the redo test of test_gpu_parity builds them."""
    pos = synth.positions(900000, n, BOX).copy()
    kind, axis = rng.integers(0, 3, n), rng.integers(0, 3, n)
    u = rng.uniform(0.01, 0.29, n).astype(np.float32)
    for i in range(n):
        pos[i, axis[i]] = (-0.0, np.float32(BOX) * (np.float32(1) + u[i]), -np.float32(BOX) * u[i])[kind[i]]
    return pos


def noted_by_kernel(pos, g):
    """Per particle: +1 the fast kernel certainly notes it, 0 certainly not, -1 undetermined (k1_edges_np.note_state
    for the entries that reach the projection; the domain test for raw coordinates outside [+0, box])."""
    raw = np.asarray(pos, np.float32)
    off = (np.signbit(raw) | (raw > np.float32(g.box)) | np.isnan(raw)).any(axis=1)
    e = ke.Entries(raw, g)
    state = ke.note_state(e, g, SERIES_MAX9)
    # only entries in a slab that the f32 pre-test lets through reach the projection: certainly those inside the
    # field, certainly not those 2 % beyond the limit (the pre-test's margins are 3e-5 and 0.8 %)
    reach = (e.plane >= 0) & (np.maximum(np.abs(e.dec), np.abs(e.ra)) <= 1.02 * g.lim)
    sure_reach = (e.plane >= 0) & e.inside
    out = np.where(reach, np.where((state == 1) & sure_reach, 1, np.where(state == 0, 0, -1)), 0)
    return np.where(off, 1, out)


@functools.lru_cache(maxsize=None)
def clean_pool():
    g = ke.Geometry.from_params(FIXTURE["a_params"])
    pos = synth.positions(0, 60000, g.box)
    return pos[noted_by_kernel(pos, g) == 0]


@functools.lru_cache(maxsize=None)
def noted_pool():
    g = ke.Geometry.from_params(FIXTURE["a_params"])
    pos, lab = FIXTURE["a_pos"], FIXTURE["a_label"]
    pos = pos[(lab & (ke.T | ke.R)) != 0]
    return pos[noted_by_kernel(pos, g) == 1]


def exception_case(n_noted, how, where, extra=None):
    """Batches of BATCH particles; the special one holds exactly n_noted noted particles, the others none."""
    g = ke.Geometry.from_params(FIXTURE["a_params"])
    rng = np.random.default_rng(100 * n_noted + len(how) + len(where))
    clean = clean_pool()
    n_dom = {"domain": n_noted, "decide": 0, "mix": n_noted // 2}[how]
    special = np.concatenate([off_domain(n_dom, rng), noted_pool()[:n_noted - n_dom]])
    assert len(special) == n_noted
    if extra is not None:
        special = np.concatenate([special[:-1], extra])
    length = {"first": BATCH, "between": BATCH, "last": 1999}[where]  # last: ragged, no multiple of 4, under a round
    batch = clean[:length].copy()
    batch[np.sort(rng.choice(length, n_noted, replace=False))] = special
    rest = clean[BATCH:]
    parts = {"first": [batch, rest[:2 * BATCH + 77]], "between": [rest[:BATCH], batch, rest[BATCH:2 * BATCH]],
             "last": [rest[:2 * BATCH], batch]}[where]
    pos = np.concatenate(parts)
    w = {"first": 0, "between": 1, "last": 2}[where]
    noted = noted_by_kernel(pos, g)
    assert not (noted == -1).any()
    per_batch = [int(noted[b:b + BATCH].sum()) for b in range(0, len(pos), BATCH)]
    assert per_batch[w] == n_noted and sum(per_batch) == n_noted, per_batch
    return g, pos


@pytest.mark.parametrize("where", ["first", "between", "last"])
@pytest.mark.parametrize("how", ["domain", "decide", "mix"])
@pytest.mark.parametrize("n_noted", [1, 255, 256, 257])
def test_exception_list_at_its_capacity(S, n_noted, how, where):
    """Exactly n_noted particles of one workgroup's batch (bin_batch = 4096) are noted for the exact epilogue -- by the
    domain test, by decide_emit (entries on a rounding tie or in the border ring, from the fixture) or both: up to 256
    fit the LDS list, 257 make the workgroup discard its records and redo the batch.  How many the kernel notes is
    asserted on the host from its documented conditions; the oracle decides the result."""
    g, pos = exception_case(n_noted, how, where)
    ps = make_pass(g.npix, g.fov, g.rnd, edges=g.edges)
    const = Expect(ps, pos)
    hydro = Expect(ps, pos, exact_masses(len(pos), np.random.default_rng(n_noted)))
    for ex, ngp, opts in ((const, False, dict(k1_stack=0)), (const, False, dict(k1_stack=1)), (const, True, {}),
                          (hydro, False, {})):
        out, mask = run(S, ex, ngp=ngp, bin_batch=BATCH, **opts)
        check(ex, out, mask, ngp=ngp, tag=f"noted {n_noted} {how} {where} {opts}")
    # (constant mass, no wave stacks, four planes of 512^2: the pass qualifies for the two-level sort at this batch size)
    out, mask = run(S, const, ngp=False, bin_batch=BATCH, k1_stack=0, sort2=1)
    assert mask & (1 << 7), f"the two-level sort did not run: mask {mask:#x}"
    check(const, out, mask, ngp=False, sort2=True, tag=f"noted {n_noted} {how} {where} sort2")


@pytest.mark.parametrize("n_noted", [3, 257])
def test_negativity_guard_from_the_exact_epilogue(S, n_noted):
    """One noted particle whose transformed coordinate is negative (raw -2.6 box on an axis that is not mirrored, as
    test_guard_negative_coordinate_returns_1 has it): plane_read raises code 1 from the epilogue of the list (3 noted)
    and of the redone batch (257)."""
    bad = np.array([[500.0, -2600.0, 500.0]], np.float32)
    g, pos = exception_case(n_noted, "domain", "first", extra=bad)
    x, y, z = oracle.transform(bad, g.box, g.sgn, g.face, g.center, g.rcase)
    assert oracle.min_guard(x, y, z) != 0
    ex = Expect(make_pass(g.npix, g.fov, g.rnd, edges=g.edges), pos)
    with pytest.raises(slicer_amd.SlicerError) as err:
        run(S, ex, ngp=True, bin_batch=BATCH)
    assert err.value.code == slicer_amd.api.ERR_NEGATIVE_COORD
    assert S.algo_mask() & FAST and not S.algo_mask() & GENERAL


# ---- D. chunk ends and alignment --------------------------------------------------------------------------------
CHUNK_LENGTHS = [1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 3]


@functools.lru_cache(maxsize=None)
def chunk_positions():
    """Particles inside the field of every plane: one read past a chunk's end changes the maps."""
    g = ke.Geometry.from_params(FIXTURE["a_params"])
    pos = synth.positions(0, 40000, BOX)
    e = ke.Entries(pos, g)
    pos = pos[e.selected]
    assert len(pos) > 2 * BATCH + 3 + 64
    return g, pos


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset12"])
@pytest.mark.parametrize("n", CHUNK_LENGTHS)
def test_chunk_lengths_and_alignment(S, n, offset):
    """A device-resident chunk of n particles (bin_batch = 4096: whole rounds, ragged rounds, one batch and a bit),
    at the start of its allocation and 12 bytes in (not 16-byte aligned); the allocation goes on with particles that
    would all be selected.  The fast kernel runs at every length, 1 included."""
    g, pool = chunk_positions()
    ex = Expect(make_pass(g.npix, g.fov, g.rnd, edges=g.edges), pool[offset:offset + n])
    d = S.to_device(pool[:offset + n + 64])

    def deposit(S, ex):
        S.deposit_device(ex.ptype, d + 12 * offset, n)

    try:
        for ngp in (False, True):
            out, mask = run(S, ex, ngp=ngp, deposit=deposit, bin_batch=BATCH)
            assert check(ex, out, mask, ngp=ngp, tag=f"n {n} offset {offset}") == n
    finally:
        S.free(d)


def test_two_odd_chunks_of_one_file(S):
    g, pool = chunk_positions()
    n1, n2 = 2 * BATCH + 3, 1333
    ex = Expect(make_pass(g.npix, g.fov, g.rnd, edges=g.edges), pool[:n1 + n2])
    d = S.to_device(pool[:n1 + n2 + 64])

    def deposit(S, ex):
        S.deposit_device(ex.ptype, d, n1)
        S.deposit_device(ex.ptype, d + 12 * n1, n2)  # (12 n1 is no multiple of 16)

    try:
        for ngp in (False, True):
            out, mask = run(S, ex, ngp=ngp, deposit=deposit, bin_batch=BATCH)
            assert check(ex, out, mask, ngp=ngp, tag="two chunks") == n1 + n2
    finally:
        S.free(d)
