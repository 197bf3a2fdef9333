"""The ray-tracing contract without a device: the restatement tests/rays_np.py against a plain
per-ray loop, the cases whose answer is known in closed form (one plane on the nodes, integer and half-pixel shifts,
the Born limit), NaN containment, slicer_lensing_plane_strengths against slicer_lensing_weights, and the refusals of
the new functions that need no device."""
import ctypes as C

import numpy as np
import pytest

import deflection_np
import rays_np as R
import shear_np
import slicer_amd
from slicer_amd import lensing
from slicer_amd.api import SlicerError

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6
D = R.D


def _err():
    return (L.slicer_last_error(None) or b"").decode()


@pytest.mark.parametrize("n_planes", [1, 2, 3])
@pytest.mark.parametrize("n", range(1, 10))
def test_restatement_equals_the_scalar_loop(n, n_planes):
    rng = np.random.default_rng(100 * n + n_planes)
    d = 1.3e-4
    planes = R.noise_planes(rng, n, n_planes, d)
    chis = [1.0, 2.5, 3.7][:n_planes]
    s, out = R.trace(n, d, chis, planes, 5.0)
    s_ref, out_ref = R.scalar_trace(n, d, chis, planes, 5.0)
    assert R.same_bits(s, s_ref) and R.same_bits(out, out_ref)
    if n >= 3 and n_planes >= 2:  # deflections of several pixels: some rays left the grid and wrapped
        before = R.trace(n, d, chis[:-1], planes[:-1])
        u = R._advance(before[R.B1], before[R.T1], R.weight(chis[-1], chis[-2])) + (n - 1) / 2.0
        assert (u < 0).any() or (u >= n).any()


def test_one_plane_on_the_nodes():
    """A = I - w_s U and delta = w_s alpha.  Bounds: the f32 rounding of the output, 2^-24 |ref|, and the f64 roundings
    in front of it: four of size 2^-53 for the matrix (1 - U, - 1, the two of the advance; the entries are of order 1),
    eight of size 2^-53 (h + |alpha| / d) d for the deflection, whose intermediate values are pixel positions."""
    n, d = 37, 1.3e-4
    rng = np.random.default_rng(7)
    a1, a2, k, g1, g2 = R.noise_planes(rng, n, 1, d)[0]
    chi, chi_s = 2.0, 5.0
    ws = (chi_s - chi) / chi_s
    _, out = R.trace(n, d, [chi], [(a1, a2, k, g1, g2)], chi_s)
    for got, m in ((out[R.KAPPA], k), (out[R.GAMMA1], g1), (out[R.GAMMA2], g2)):
        ref = ws * m.astype(np.float64)
        assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + 4 * 2.0 ** -53)
    assert np.all(out[R.OMEGA] == 0)
    h = (n - 1) / 2.0
    for got, a in ((out[R.DEFLECTION1], a1), (out[R.DEFLECTION2], a2)):
        ref = ws * a.astype(np.float64)
        assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref) + 8 * 2.0 ** -53 * (h * d + np.abs(a)))


SHIFTS = [(3, -2), (None, None)]  # None: (n + 1, -n - 3)


@pytest.mark.parametrize("half", [(0, 0), (0.5, 0), (0, 0.5), (0.5, 0.5)])
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [8, 9])
def test_integer_and_half_pixel_shifts(n, shift, half):
    s1, s2 = (n + 1, -n - 3) if shift[0] is None else shift
    s1, s2 = s1 + half[0], s2 + half[1]
    planes, ref = R.shift_case(n, s1, s2)
    _, out = R.trace(n, D, [1.0, 2.0], planes, 4.0)
    assert R.same_bits(out, ref)
    assert np.array_equal(out[R.GAMMA2].view(np.uint32), ref[R.GAMMA2].view(np.uint32))  # the zeros' signs included


def smooth_planes(n, angle_deg, eps, seed=3):
    """Three band-limited lens maps of rms eps with their spectral alpha and gamma (tests/shear_np, deflection_np)."""
    rng = np.random.default_rng(seed)
    k0 = np.fft.fftfreq(n)[:, None] * n
    k1 = np.fft.rfftfreq(n)[None, :] * n
    planes, lens = [], []
    for _ in range(3):
        white = np.fft.rfft2(rng.standard_normal((n, n)))
        lm = np.fft.irfft2(white * np.exp(-(k0 ** 2 + k1 ** 2) / (2 * 3.0 ** 2)), s=(n, n))
        lm = (lm - lm.mean()) / lm.std() * eps
        sh = shear_np.shear(lm, angle_deg)
        al = deflection_np.deflection(lm, angle_deg)
        planes.append([m.astype(np.float32) for m in (al[0], al[1], lm, sh["gamma1"], sh["gamma2"])])
        lens.append(lm)
    return planes, lens


def test_born_limit():
    """Ray kappa minus Born kappa is second order in the lens strength: it falls fourfold when the maps are halved.
    Rotation needs two planes and is second order too."""
    n, angle = 64, 2.0
    d = np.deg2rad(angle) / n
    chis, chi_s = [1.0, 2.0, 3.0], 4.0
    diff, omega = [], []
    for eps in (0.02, 0.01, 0.005):
        planes, lens = smooth_planes(n, angle, eps)
        _, out = R.trace(n, d, chis, planes, chi_s)
        born = sum((chi_s - c) / chi_s * lm for c, lm in zip(chis, lens))
        diff.append(np.abs(out[R.KAPPA] - born).max())
        omega.append(np.abs(out[R.OMEGA]).max())
    print("kappa_ray - kappa_Born:", diff, "ratios:", diff[0] / diff[1], diff[1] / diff[2], "max|omega|:", omega)
    assert 3 <= diff[0] / diff[1] <= 5 and 3 <= diff[1] / diff[2] <= 5
    assert omega[0] > 0
    _, one = R.trace(n, d, chis[:1], smooth_planes(n, angle, 0.02)[0][:1], chi_s)
    assert np.all(one[R.OMEGA] == 0)


@pytest.mark.parametrize("which", range(5))
def test_a_nan_pixel_reaches_exactly_the_rays_that_read_it(which):
    n, d = 12, 1.3e-4
    rng = np.random.default_rng(11 + which)
    planes = R.noise_planes(rng, n, 2, d, shift_pixels=0.4)
    clean = R.trace(n, d, [1.0, 2.0], planes)
    a, b = 0, 5  # a pixel of the first row: two of the rays that read it come from the last row, around the seam
    planes[0][which] = planes[0][which].copy()
    planes[0][which][a, b] = np.nan
    first = R.trace(n, d, [1.0], planes[:1])
    hit = np.isnan(first).any(axis=0)
    expect = np.zeros((n, n), bool)
    for i in (a, a - 1):
        for j in (b, b - 1):
            expect[i % n, j % n] = True  # on the nodes ray (i, j) reads pixels (i, j) ... (i + 1, j + 1)
    assert np.array_equal(hit, expect)
    both = R.trace(n, d, [1.0, 2.0], planes)
    if which < 2:  # a NaN deflection: the ray's position is NaN at the next plane, and with it all it reads there
        assert np.all(np.isnan(both[:, expect][[R.T1, R.T2, R.T11, R.T12, R.T21, R.T22]]))
    assert np.array_equal(np.isnan(both).any(axis=0), expect)
    assert R.same_bits(both[:, ~expect], clean[:, ~expect])


CONE = dict(ld=np.arange(10) * 50.0, ld2=np.arange(10) * 50.0 + 50.0, zsnap=np.repeat([0.0, 0.1], 5))


@pytest.mark.parametrize("sources", ["all", [0.05, 0.12, 0.19]])
@pytest.mark.parametrize("w0", [-1.0, -1.3])
def test_plane_strengths_give_the_born_weights(w0, sources):
    args = (0.3, 0.7, w0, 5.0, 64, CONE["ld"], CONE["ld2"], CONE["zsnap"])
    w = slicer_amd.plane_weights(*args, sources=sources)
    p = slicer_amd.plane_strengths(*args, sources=sources)
    assert np.array_equal(p["chil"], w["chil"]) and np.array_equal(p["zs"], w["zs"])
    chis, chil = p["chis"][:, None], p["chil"][None, :]
    c = p["strength"][None, :] * (chis - chil) / chis
    live = w["c"] != 0
    rel = np.abs(c - w["c"])[live] / np.abs(w["c"][live])
    print("worst |strength (chi_s - chi_p) / chi_s - c_sp| / |c_sp| in units of 2^-53:", rel.max() / 2.0 ** -53)
    assert rel.max() <= 4 * 2.0 ** -53
    # the planes in front of a source: z(ld2) <= zs + 1e-4, the planes that carry a weight
    assert np.array_equal(p["n_in_front"], live.sum(axis=1))
    assert np.array_equal(p["n_in_front"], [(w["zup"] <= z + 1e-4).sum() for z in p["zs"]])
    assert np.all(np.diff(p["chil"]) > 0) and np.all(p["chis"] > 0)


def test_n_in_front_rule_at_the_edge():
    args = (0.3, 0.7, -1.0, 5.0, 64, CONE["ld"], CONE["ld2"], CONE["zsnap"])
    zup = slicer_amd.plane_weights(*args)["zup"]
    p = slicer_amd.plane_strengths(*args, sources=[zup[3] - 0.99e-4, zup[3] - 1.01e-4, 1e-6, zup[9] + 1.0])
    assert list(p["n_in_front"]) == [4, 3, 0, 10]
    # growth off: g = 1 for every plane; the first five planes are cut from the z = 0 snapshot and lie behind it, g < 1
    on, off = slicer_amd.plane_strengths(*args)["strength"], slicer_amd.plane_strengths(*args, growth=False)["strength"]
    assert np.all(on[:5] < off[:5]) and np.all(off > 0)


def test_plane_strengths_refusals():
    ld, ld2, zs = [0.0, 50.0], [50.0, 100.0], [0.0, 0.0]
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_strengths(0.3, 0.6, -1.0, 2.0, 32, ld, ld2, zs)  # curved
    assert e.value.code == ERR_UNSUPPORTED and "flat" in str(e.value)
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_strengths(0.3, 0.7, -1.0, 2.0, 32, ld, ld2, zs, physical=True)
    assert e.value.code == ERR_UNSUPPORTED
    for bad in (dict(omega_m=0.0, omega_lambda=1.0), dict(fov_deg=0.0), dict(fov_deg=180.0), dict(npix=0)):
        kw = dict(omega_m=0.3, omega_lambda=0.7, w0=-1.0, fov_deg=2.0, npix=32, ld=ld, ld2=ld2, zsnap=zs)
        kw.update(bad)
        with pytest.raises(SlicerError) as e:
            slicer_amd.plane_strengths(**kw)
        assert e.value.code == ERR_ARG and "slicer_lensing_plane_strengths" in str(e.value)
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_strengths(0.3, 0.7, -1.0, 2.0, 32, [50.0, 0.0], [40.0, 50.0], zs)  # edges out of order
    assert e.value.code == ERR_ARG and "out of order" in str(e.value)
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_strengths(0.3, 0.7, -1.0, 2.0, 32, ld, ld2, [0.0, -1.0])
    assert e.value.code == ERR_ARG
    # a NULL strength array; no source list with a source count that is not the plane count
    a = np.array(ld), np.array(ld2), np.array(zs)
    out = np.zeros(2)
    call = lambda n_src, strength: L.slicer_lensing_plane_strengths(  # noqa: E731
        0.3, 0.7, -1.0, 0.0, 2.0, 32, 1, 0, 2, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, n_src, None, strength,
        None, None, None)
    assert call(2, out.ctypes.data) == 0 and np.all(out > 0)
    assert call(2, None) == ERR_ARG
    assert call(3, out.ctypes.data) == ERR_ARG


@pytest.mark.parametrize("npix, spacing, code, text", [
    (0, 1e-4, ERR_ARG, "npix"),
    (-3, 1e-4, ERR_ARG, "npix"),
    (131073, 1e-4, ERR_UNSUPPORTED, "131072"),
    (16, 0.0, ERR_ARG, "spacing"),
    (16, -1e-4, ERR_ARG, "spacing"),
    (16, np.inf, ERR_ARG, "spacing"),
    (16, np.nan, ERR_ARG, "spacing"),
    (16, 1e-4, ERR_ARG, "null"),  # good numbers: the missing handle
])
def test_create_refusals_need_no_device(npix, spacing, code, text):
    out = C.c_void_p(1)
    assert L.slicer_rays_create(None, npix, spacing, C.byref(out)) == code
    assert text in _err()
    assert out.value is None
    assert L.slicer_rays_create(None, npix, spacing, None) == code


def test_refusals_of_the_other_calls_need_no_device():
    buf = np.zeros(4, np.float32)
    p = buf.ctypes.data
    for chi in (np.nan, np.inf, -np.inf):
        assert L.slicer_rays_step(None, chi, p, p, p, p, p) == ERR_ARG and "finite" in _err()
    for k in range(5):
        maps = [p] * 5
        maps[k] = None
        assert L.slicer_rays_step(None, 1.0, *maps) == ERR_ARG and "null map" in _err()
    assert L.slicer_rays_step(None, 1.0, p, p, p, p, p) == ERR_ARG and "null handle" in _err()
    outs = (C.c_void_p * 6)(*[p] * 6)
    for chi_s in (0.0, -1.0, np.nan, np.inf):
        assert L.slicer_rays_observe(None, chi_s, outs) == ERR_ARG and "positive" in _err()
    assert L.slicer_rays_observe(None, 1.0, (C.c_void_p * 6)()) == ERR_ARG and "every output" in _err()
    assert L.slicer_rays_observe(None, 1.0, None) == ERR_ARG
    assert L.slicer_rays_observe(None, 1.0, outs) == ERR_ARG and "null handle" in _err()
    assert L.slicer_rays_state(None, buf.ctypes.data) == ERR_ARG
    assert L.slicer_rays_planes(None, None, None) == ERR_ARG
    assert L.slicer_rays_reset(None) == ERR_ARG
    assert L.slicer_rays_destroy(None) == ERR_ARG
    assert L.slicer_kappa_reset(None) == ERR_ARG
