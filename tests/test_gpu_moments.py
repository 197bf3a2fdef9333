"""slicer_moments_* on the device against the restatement tests/moments_np.py: the halved maps
bit for bit, the sums and means inside the counted bounds, exact integer sums, the bitwise invariants, the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import moments_np as M
import slicer_amd
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
LD = np.longdouble
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 100, 1000, 1023, 1024, 4096]


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


def full(n):
    return int(np.log2(n))


@functools.lru_cache(maxsize=None)
def make_map(n, kind, seed=0):
    rng = np.random.default_rng(7919 * n + seed)
    g = rng.standard_normal((n, n))
    if kind == "white":
        x = g
    elif kind == "lognormal":
        x = np.exp(g) - np.exp(0.5)
    elif kind == "offset":
        x = 1.0 + 1e-3 * g
    elif kind == "mass":
        x = 1e10 * np.exp(g)
    elif kind == "normalised":  # magnitudes 0.5 ... 2 of either sign: no sum of four is subnormal
        x = rng.uniform(0.5, 2.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
    elif kind == "integers":
        x = rng.integers(-3, 4, (n, n))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def run(s, x, levels, mode="mean", centres=None, off_grid=False, maps=True):
    """(read(), [level maps 1 ... levels]) of one run on a fresh handle."""
    n = x.shape[0]
    flat = np.concatenate([np.zeros(1, np.float32), x.ravel()]) if off_grid else x.ravel()
    d = s.to_device(flat)
    try:
        with slicer_amd.Moments(s, n, levels, mode) as m:
            m.run(d + 4 if off_grid else d, centres)
            r = m.read()
            return r, [m.read_map(l) for l in range(1, levels + 1)] if maps else None
    finally:
        s.free(d)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_read(a, b, keys=("npix", "mean", "centre", "sums")):
    return all(same_bits(a[k], b[k]) for k in keys)


def check_bounds(r, pyr, given=None):
    """Every level of the read r inside the counted bounds, against the restatement's level maps pyr."""
    assert [int(v) for v in r["npix"]] == [p.shape[0] for p in pyr]
    for l, x in enumerate(pyr):
        n = x.shape[0]
        mean, mean_abs = M.mean_ld(x)
        err = abs(LD(r["mean"][l]) - mean)
        print(f"level {l} n {n}: mean error / bound = {float(err / M.mean_bound(mean_abs, n)) if mean_abs else 0.0:.3g}")
        assert err <= M.mean_bound(mean_abs, n), (l, n)
        c = r["centre"][l]
        if given is None or np.isnan(given[l]):
            assert c == r["mean"][l]
        else:
            assert c == given[l]
        ref, A = M.sums_ld(x, c)
        bound = M.sum_bounds(A, n)
        err = np.abs(r["sums"][l].astype(LD) - ref)
        print(f"level {l} n {n}: sum errors / bounds = {np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)}")
        assert np.all(err <= bound), (l, n)
        assert same_bits(r["moments"][l], r["sums"][l] / float(n) ** 2)


@pytest.mark.parametrize("mode", ["mean", "sum"])
@pytest.mark.parametrize("n", SIZES)
def test_halved_maps_are_the_restatement_bit_for_bit(slicer, n, mode):
    x = make_map(n, "normalised")
    r, maps = run(slicer, x, full(n), mode)
    pyr = M.pyramid(x, full(n), mode)
    assert len(maps) == len(pyr) - 1
    for got, ref in zip(maps, pyr[1:]):
        assert same_bits(got, ref), ref.shape
    assert [int(v) for v in r["npix"]] == [n >> l for l in range(full(n) + 1)]


@pytest.mark.parametrize("centres", ["own", "given", "mixed"])
@pytest.mark.parametrize("n", [5, 66, 257, 1000])
def test_sums_and_means_are_inside_the_bounds(slicer, n, centres):
    levels = full(n)
    for kind in ("white", "lognormal", "offset"):
        x = make_map(n, kind)
        pyr = M.pyramid(x, levels, "mean")
        given = None
        if centres != "own":
            given = np.array([float(M.mean_ld(p)[0]) * 1.01 + 1e-3 for p in pyr])
            if centres == "mixed":
                given[levels // 2] = np.nan
        r, maps = run(slicer, x, levels, "mean", given)
        assert all(same_bits(a, b) for a, b in zip(maps, pyr[1:]))
        check_bounds(r, pyr, given)


@pytest.mark.parametrize("n", [33, 1000])
def test_block_sums_of_a_mass_like_map(slicer, n):
    x = make_map(n, "mass")
    pyr = M.pyramid(x, full(n), "sum")
    r, maps = run(slicer, x, full(n), "sum")
    assert all(same_bits(a, b) for a, b in zip(maps, pyr[1:]))
    assert pyr[-1].max() > 1e10 * n  # the levels grow: these are sums
    check_bounds(r, pyr)


@pytest.mark.parametrize("n", [5, 16, 33, 1000])
def test_integer_maps_give_the_integer_sums_exactly(slicer, n):
    x = make_map(n, "integers")
    given = np.array([1.0, 2.0])
    r, maps = run(slicer, x, 1, "sum", given)
    pyr = M.pyramid(x, 1, "sum")
    assert same_bits(maps[0], pyr[1])
    for l in range(2):
        d = pyr[l].astype(np.int64) - int(given[l])
        exact = [int((d ** k).sum()) for k in M.ORDERS]
        assert max(abs(v) for v in exact) < 2 ** 53
        assert [float(v) for v in exact] == list(r["sums"][l])
        assert r["mean"][l] == float(pyr[l].astype(np.int64).sum()) / pyr[l].size


@pytest.mark.parametrize("given", [False, True])
def test_a_constant_map_has_no_moments(slicer, given):
    n, c = 33, 0.375
    x = np.full((n, n), c, np.float32)
    r, maps = run(slicer, x, full(n), "mean", np.full(full(n) + 1, c) if given else None)
    assert all(np.all(m == np.float32(c)) for m in maps)
    assert np.all(r["mean"] == c) and np.all(r["centre"] == c)
    assert np.all(r["sums"] == 0.0)


@pytest.mark.parametrize("n", [9, 66, 1000])
def test_a_level_of_the_pyramid_is_bitwise_that_level_alone(slicer, n):
    x = make_map(n, "lognormal")
    levels = full(n)
    r, maps = run(slicer, x, levels)
    given = r["mean"] * 0.99 + 1e-4
    rg, _ = run(slicer, x, levels, centres=given, maps=False)
    for l in range(levels + 1):
        xl = x if l == 0 else maps[l - 1]
        alone, _ = run(slicer, xl, 0)
        for k in ("mean", "centre", "sums"):
            assert same_bits(alone[k][0], r[k][l]), (l, k)
        # a given centre: the sums bitwise; level 0's mean then comes out of the moment pass's own tree (still bounded)
        alone, _ = run(slicer, xl, 0, centres=given[l:l + 1])
        assert same_bits(alone["sums"][0], rg["sums"][l]) and alone["centre"][0] == given[l] == rg["centre"][l]
        mean, mean_abs = M.mean_ld(xl)
        assert abs(LD(alone["mean"][0]) - mean) <= M.mean_bound(mean_abs, xl.shape[0])
        if l == 0:
            assert same_bits(alone["mean"][0], rg["mean"][0])


@pytest.mark.parametrize("n", [64, 1024])
def test_an_input_off_the_16_byte_grid_gives_the_same_bits(slicer, n):
    x = make_map(n, "lognormal")
    for centres in (None, np.full(full(n) + 1, 0.25)):
        r, maps = run(slicer, x, full(n), centres=centres)
        r_off, maps_off = run(slicer, x, full(n), centres=centres, off_grid=True)
        assert same_read(r, r_off)
        assert all(same_bits(a, b) for a, b in zip(maps, maps_off))


def test_two_runs_are_bitwise_equal_and_leave_the_input_alone(slicer):
    n = 257
    x = make_map(n, "white")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Moments(slicer, n, full(n)) as m:
            m.run(d)
            first = m.read()
            first_maps = [m.read_map(l) for l in range(1, full(n) + 1)]
            m.run(d, np.full(full(n) + 1, 0.5))  # (another state in between)
            m.run(d)
            assert same_read(first, m.read())
            assert all(same_bits(a, m.read_map(l + 1)) for l, a in enumerate(first_maps))
        assert same_bits(slicer.to_host(d, (n, n), np.float32), np.asarray(x))
    finally:
        slicer.free(d)


def test_run_kappa_is_run_on_the_kappa_map(slicer):
    n = 48
    x = make_map(n, "lognormal")
    d = slicer.to_device(x)
    try:
        with slicer_amd.Kappa(slicer, n, 1) as kappa, slicer_amd.Moments(slicer, n, 3) as m:
            kappa.add_device([d], [[1.0]])
            m.run_kappa(kappa, 0)
            a = m.read()
            m.run(kappa.device_map(0))
            assert same_read(a, m.read())
            check_bounds(a, M.pyramid(kappa.read(0), 3))
    finally:
        slicer.free(d)


def test_combine_moments_is_the_average_of_moment_py(slicer):
    n, levels = 100, 2
    maps = [make_map(n, "lognormal", seed) for seed in range(3)]
    pyrs = [M.pyramid(x, levels) for x in maps]
    centres = np.array([np.mean([float(M.mean_ld(p[l])[0]) for p in pyrs]) for l in range(levels + 1)])
    reads = [run(slicer, x, levels, centres=centres, maps=False)[0] for x in maps]
    got = slicer_amd.combine_moments(reads)
    assert got.shape == (levels + 1, 7)
    for l in range(levels + 1):
        nl = n >> l
        assert same_bits(got[l], (reads[0]["sums"][l] + reads[1]["sums"][l] + reads[2]["sums"][l]) / 3 / float(nl) ** 2)
        ref, bound = LD(0), LD(0)
        for p in pyrs:  # m = sum_f np.sum((kappa - mean) ** i) / len(files) / kappa.size
            s, A = M.sums_ld(p[l], centres[l])
            ref, bound = ref + s, bound + M.sum_bounds(A, nl)
        scale = LD(3) * nl * nl
        assert np.all(np.abs(got[l].astype(LD) - ref / scale) <= (bound / scale) * (1 + 2.0 ** -20) + 3 * M.U * np.abs(ref / scale))


def test_state_and_level_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    mh, p = C.c_void_p(), C.c_void_p()
    assert L.slicer_moments_create(slicer._h, n, 2, 0, C.byref(mh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        buf = np.zeros(3 * 7)
        assert L.slicer_moments_read(mh, None, None, None, buf.ctypes.data) == ERR_STATE
        assert err() == "slicer_moments_read before any slicer_moments_run"
        assert L.slicer_moments_device_map(mh, 1, C.byref(p)) == ERR_STATE
        assert err() == "slicer_moments_device_map before any slicer_moments_run"
        assert L.slicer_moments_run(mh, None, None) == ERR_ARG
        assert err() == "slicer_moments_run: null argument"
        assert L.slicer_moments_run(mh, d, None) == 0
        assert L.slicer_moments_read(mh, None, None, None, buf.ctypes.data) == 0
        for level in (0, 3, -1):
            assert L.slicer_moments_device_map(mh, level, C.byref(p)) == ERR_ARG
            assert err() == f"slicer_moments_device_map: level = {level} outside 1..2"
            assert not p.value
            assert L.slicer_moments_read_map(mh, level, buf.ctypes.data) == ERR_ARG
        assert L.slicer_moments_device_map(mh, 2, C.byref(p)) == 0 and p.value
        out = C.c_void_p(1)
        assert L.slicer_moments_create(slicer._h, n, 5, 0, C.byref(out)) == ERR_ARG
        assert err() == "slicer_moments_create: levels = 5 outside 0..4 for npix = 16"
        assert not out.value
        assert L.slicer_moments_create(slicer._h, n, 2, 0, None) == ERR_ARG
        assert err() == "slicer_moments_create: null argument"
    finally:
        L.slicer_moments_destroy(mh)
        slicer.free(d)


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n, "white"))
    try:
        with slicer_amd.Moments(slicer, n, 2) as m:
            slicer.profile_reset()
            slicer.profile_enable(True)
            m.run(d)
            m.run(d, [0.0, 0.0, 0.0])
            m.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["moments"][0] == 2 and prof["moments_sum"][0] == 1
    finally:
        slicer.free(d)
