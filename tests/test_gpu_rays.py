"""Device ray tracing (slicer_rays_*) against the numpy restatement in tests/rays_np.py, bit for
bit: the state (slicer_rays_state) and the six outputs (slicer_rays_observe).  Also Kappa.reset."""
import ctypes as C

import numpy as np
import pytest

import rays_np as R
import shear_np
import slicer_amd
from slicer_amd import lensing
from slicer_amd.api import SlicerError

L = lensing._L
ERR_ARG = 2
ALL = tuple(range(slicer_amd.RAYS_COUNT))


class DeviceMaps:
    """f32 maps on the device, each optionally `off` floats past the start of its own allocation."""

    def __init__(self, s, maps, off=0):
        self.s, self.off = s, off
        self.hosts = [np.ascontiguousarray(m, np.float32) for m in maps]
        self.base = [s.to_device(np.concatenate([np.zeros(off, np.float32), m.ravel()])) for m in self.hosts]
        self.ptrs = [b + 4 * off for b in self.base]

    def read(self):
        return [self.s.to_host(p, m.shape, np.float32) for p, m in zip(self.ptrs, self.hosts)]

    def free(self):
        for b in self.base:
            self.s.free(b)


def observe_off(s, rays, chi_s, which=ALL, off=0):
    """Rays.observe into buffers `off` floats past the start of their allocations."""
    n = rays.npix
    base = {w: s.malloc(4 * (n * n + off)) for w in which}
    try:
        rays.observe_device(chi_s, [base[w] + 4 * off if w in base else None for w in ALL])
        return {w: s.to_host(base[w] + 4 * off, (n, n), np.float32) for w in which}
    finally:
        for b in base.values():
            s.free(b)


def device_trace(s, n, d, chis, planes, chi_s, map_off=0, out_off=0, check_inputs=False):
    """(state, [6, n, n] outputs) of a fresh handle."""
    with slicer_amd.Rays(s, n, d) as rays:
        held = []
        try:
            for chi, maps in zip(chis, planes):
                dm = DeviceMaps(s, maps, map_off)
                held.append(dm)
                rays.step(chi, *dm.ptrs)
            out = observe_off(s, rays, chi_s, ALL, out_off)
            state = rays.state()
            if check_inputs:
                for dm in held:
                    for got, m in zip(dm.read(), dm.hosts):
                        assert R.same_bits(got, m)
            return state, np.stack([out[w] for w in ALL])
        finally:
            for dm in held:
                dm.free()


def smooth_planes(n, n_planes, d):
    """Slowly varying maps: deflections below a pixel, so neighbouring rays stay neighbours."""
    i = np.arange(n)[:, None] / n
    j = np.arange(n)[None, :] / n
    planes = []
    for p in range(n_planes):
        a1 = 0.7 * d * np.sin(2 * np.pi * (i + 2 * j) + p)
        a2 = 0.6 * d * np.cos(2 * np.pi * (2 * i - j) + 0.3 * p)
        k = 0.05 * np.cos(2 * np.pi * (i + j) + p)
        g1 = 0.04 * np.sin(2 * np.pi * (3 * i - j) + p)
        g2 = 0.03 * np.sin(2 * np.pi * (i - 2 * j) + 2 * p)
        planes.append([(m + np.zeros((n, n))).astype(np.float32) for m in (a1, a2, k, g1, g2)])
    return planes


CHIS = [1.0, 2.5, 3.7, 4.1, 6.0]
CASES = [(n, p) for n in (1, 2, 3, 5, 16, 17, 63, 64, 65, 100, 129) for p in (1, 2, 3, 5)] + [(1000, 3), (1024, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_planes", CASES)
def test_matches_restatement(n, n_planes):
    d, chis, chi_s = 1.3e-4, CHIS[:n_planes], 7.5
    rng = np.random.default_rng(1000 * n + n_planes)
    with slicer_amd.Slicer(0) as s:
        for label, planes in (("white", R.noise_planes(rng, n, n_planes, d)), ("smooth", smooth_planes(n, n_planes, d))):
            ref_s, ref_o = R.trace(n, d, chis, planes, chi_s)
            got_s, got_o = device_trace(s, n, d, chis, planes, chi_s, check_inputs=True)
            for k, name in enumerate(R.STATE):
                assert R.same_bits(got_s[k], ref_s[k]), f"{label}: state {name}"
            for k in ALL:
                assert R.same_bits(got_o[k], ref_o[k]), f"{label}: output {k}"
            if label == "white" and n >= 3 and n_planes >= 2:  # some rays left the grid and wrapped
                u = ref_s[R.B1] + (n - 1) / 2.0
                assert (u < 0).any() or (u >= n).any()


@pytest.mark.gpu
@pytest.mark.parametrize("half", [(0, 0), (0.5, 0), (0, 0.5), (0.5, 0.5)])
@pytest.mark.parametrize("shift", [(3, -2), (None, None)])
@pytest.mark.parametrize("n", [8, 9, 130])
def test_integer_and_half_pixel_shifts(n, shift, half):
    s1, s2 = (n + 1, -n - 3) if shift[0] is None else shift
    planes, ref = R.shift_case(n, s1 + half[0], s2 + half[1])
    with slicer_amd.Slicer(0) as s:
        _, out = device_trace(s, n, R.D, [1.0, 2.0], planes, 4.0)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 17, 64])
def test_pointers_off_the_16_byte_grid_and_output_subsets(n):
    d, chis, chi_s = 1.3e-4, CHIS[:3], 7.5
    planes = R.noise_planes(np.random.default_rng(n), n, 3, d)
    with slicer_amd.Slicer(0) as s:
        state, out = device_trace(s, n, d, chis, planes, chi_s)
        for map_off, out_off in ((1, 0), (0, 1), (1, 1), (2, 2), (3, 0)):
            st2, out2 = device_trace(s, n, d, chis, planes, chi_s, map_off, out_off)
            assert R.same_bits(st2, state) and R.same_bits(out2, out)
        with slicer_amd.Rays(s, n, d) as rays:
            held = [DeviceMaps(s, maps) for maps in planes]
            for chi, dm in zip(chis, held):
                rays.step(chi, *dm.ptrs)
            for which in ((0,), (3,), (4,), (5,), (1, 2), (0, 4), (2, 3, 5), (0, 1, 2, 3)):
                for off in (0, 1):
                    part = observe_off(s, rays, chi_s, which, off)
                    for w in which:
                        assert R.same_bits(part[w], out[w]), (which, off, w)
            assert R.same_bits(rays.state(), state)
            for dm in held:
                dm.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 64])
def test_observe_leaves_the_state_and_state_rules(n):
    d = 1.3e-4
    planes = R.noise_planes(np.random.default_rng(n + 5), n, 2, d)
    with slicer_amd.Slicer(0) as s, slicer_amd.Rays(s, n, d) as rays:
        held = [DeviceMaps(s, maps) for maps in planes]
        # before any step: the start state, and an observation of zeros (gamma2's is -0.5 * 0)
        assert rays.planes() == (0, 0.0)
        assert R.same_bits(rays.state(), R.start(n))
        zero = rays.observe(3.0)
        ref0 = R.observe(R.start(n), R.weight(3.0, 0.0), d)
        for w in ALL:
            assert np.array_equal(zero[w].view(np.uint32), ref0[w].view(np.uint32)) and np.all(zero[w] == 0)
        assert R.same_bits(rays.state(), R.start(n))
        rays.step(1.0, *held[0].ptrs)
        first = rays.observe(1.5)
        rays.step(2.0, *held[1].ptrs)
        assert rays.planes() == (2, 2.0)
        got = rays.observe(4.0)
        ref_s, ref_o = R.trace(n, d, [1.0, 2.0], planes, 4.0)
        ref_1 = R.trace(n, d, [1.0], planes[:1], 1.5)[1]
        for w in ALL:
            assert R.same_bits(got[w], ref_o[w]) and R.same_bits(first[w], ref_1[w])
        assert R.same_bits(rays.state(), ref_s)
        # a source on the last plane: w = 0
        on = rays.observe(2.0)
        ref_on = R.observe(ref_s, 0.0, d)
        for w in ALL:
            assert R.same_bits(on[w], ref_on[w])
        # refusals that need the handle's state; they leave it as it was
        for chi in (2.0, 1.0, 0.0, -1.0):
            with pytest.raises(SlicerError) as e:
                rays.step(chi, *held[0].ptrs)
            assert e.value.code == ERR_ARG and "not above" in str(e.value)
        with pytest.raises(SlicerError) as e:
            rays.observe(1.999)
        assert e.value.code == ERR_ARG and "below" in str(e.value)
        with pytest.raises(SlicerError) as e:
            rays.step(3.0, held[0].ptrs[0], None, *held[0].ptrs[2:])
        assert e.value.code == ERR_ARG
        with pytest.raises(SlicerError) as e:
            rays.observe_device(4.0, [None] * 6)
        assert e.value.code == ERR_ARG and "every output" in str(e.value)
        assert L.slicer_rays_state(rays._rh, None) == ERR_ARG
        assert rays.planes() == (2, 2.0) and R.same_bits(rays.state(), ref_s)
        # reset, then the same steps: a fresh handle; and the same again: two runs are equal
        for _ in range(2):
            rays.reset()
            assert rays.planes() == (0, 0.0) and R.same_bits(rays.state(), R.start(n))
            rays.step(1.0, *held[0].ptrs)
            rays.step(2.0, *held[1].ptrs)
            again = rays.observe(4.0)
            assert R.same_bits(rays.state(), ref_s)
            for w in ALL:
                assert R.same_bits(again[w], ref_o[w])
        for dm in held:
            dm.free()


@pytest.mark.gpu
def test_nan_inf_and_runaway_rays():
    n, d = 33, 1.3e-4
    rng = np.random.default_rng(33)
    planes = R.noise_planes(rng, n, 3, d, shift_pixels=0.4)
    planes[0][2][4, 7] = np.nan      # kappa
    planes[0][0][0, 20] = np.inf     # alpha1 on the seam row
    planes[0][4][32, 32] = -np.inf   # gamma2 in the corner
    planes[1][1][10, 10] = np.nan    # alpha2, met off the nodes
    planes[0][0][20, 3] = np.float32(2.0 ** 31 * d)    # u leaves +-2^30 at the next plane
    planes[0][1][25, 9] = np.float32(-2.0 ** 40 * d)
    clean = [[m.copy() for m in maps] for maps in planes]
    clean[0][0][20, 3] = clean[0][1][25, 9] = 0.0
    chis, chi_s = CHIS[:3], 7.5
    ref_s, ref_o = R.trace(n, d, chis, planes, chi_s)
    tame_s, _ = R.trace(n, d, chis, clean, chi_s)
    with slicer_amd.Slicer(0) as s:
        got_s, got_o = device_trace(s, n, d, chis, planes, chi_s)
    assert R.same_bits(got_s, ref_s) and R.same_bits(got_o, ref_o)
    # the runaway rays are NaN, their neighbours are what they are without them
    for i, j in ((20, 3), (25, 9)):
        assert np.all(np.isnan(got_s[:, i, j][[R.T1, R.T2, R.T11, R.T12, R.T21, R.T22]]))
    nan = np.isnan(got_s).any(axis=0)
    assert nan[20, 3] and nan[25, 9] and 4 < nan.sum() < 40
    others = ~nan
    assert R.same_bits(got_s[:, others], tame_s[:, others])


@pytest.mark.gpu
@pytest.mark.parametrize("gradient", [False, True])
@pytest.mark.parametrize("n", [30, 100])
def test_step_shear_takes_the_maps_of_a_shear_handle(n, gradient):
    angle = 2.0
    d = np.deg2rad(angle) / n
    lens_maps = [0.02 * shear_np.clustered(n, n + p) for p in range(2)]
    fd = (slicer_amd.SHEAR_FD_ALPHA1, slicer_amd.SHEAR_FD_ALPHA2, slicer_amd.SHEAR_FD_KAPPA, slicer_amd.SHEAR_FD_GAMMA1,
          slicer_amd.SHEAR_FD_GAMMA2)
    sp = (slicer_amd.SHEAR_ALPHA1, slicer_amd.SHEAR_ALPHA2, None, slicer_amd.SHEAR_GAMMA1, slicer_amd.SHEAR_GAMMA2)
    with slicer_amd.Slicer(0) as s, slicer_amd.Shear(s, n, angle) as sh, slicer_amd.Rays(s, n, d) as rays:
        planes, held = [], []
        for chi, lm in zip((1.0, 2.0), lens_maps):
            lm = np.ascontiguousarray(lm, np.float32)
            dl = s.to_device(lm)
            held.append(dl)
            sh.run(dl)
            if gradient:
                sh.fd()
            else:
                sh.deflection()
            rays.step_shear(sh, chi, gradient=gradient)
            planes.append([lm if w is None else sh.read(w) for w in (fd if gradient else sp)])
        got = rays.observe(4.0)
        state = rays.state()
        for dl in held:
            s.free(dl)
    ref_s, ref_o = R.trace(n, d, [1.0, 2.0], planes, 4.0)
    assert R.same_bits(state, ref_s)
    for w in ALL:
        assert R.same_bits(got[w], ref_o[w])
    assert np.abs(got[slicer_amd.RAYS_OMEGA]).max() > 0


@pytest.mark.gpu
def test_step_shear_needs_the_maps():
    n = 30
    with slicer_amd.Slicer(0) as s, slicer_amd.Shear(s, n, 2.0) as sh, slicer_amd.Rays(s, n, 1e-3) as rays:
        with pytest.raises(ValueError):
            rays.step_shear(sh, 1.0)
        dl = s.to_device(np.zeros((n, n), np.float32))
        sh.run(dl)
        with pytest.raises(SlicerError):  # no deflection() after the run
            rays.step_shear(sh, 1.0)
        with pytest.raises(SlicerError):  # no fd() after the run
            rays.step_shear(sh, 1.0, gradient=True)
        assert rays.planes() == (0, 0.0)
        s.free(dl)


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_src", [(17, 1), (64, 3)])
def test_kappa_reset_gives_the_handle_as_created(n, n_src):
    rng = np.random.default_rng(n)
    maps = (rng.gamma(0.5, 2.0, (3, n, n)) * 3.0).astype(np.float32)
    c = rng.uniform(1e-5, 1e-3, (3, n_src))
    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(m) for m in maps]
        with slicer_amd.Kappa(s, n, n_src) as fresh:
            fresh.add_device(ptrs[1:], c[1:])
            ref = [fresh.read(k) for k in range(n_src)]
            ref_means = fresh.plane_means()
        with slicer_amd.Kappa(s, n, n_src) as k:
            k.add_device(ptrs[:2], c[:2])
            k.finalize()
            k.reset()
            assert k.n_added == 0 and k.plane_means().size == 0
            with pytest.raises(SlicerError):  # nothing finalized since the reset
                p = C.c_void_p()
                s._chk(L.slicer_kappa_device_map(k._kh, 0, C.byref(p)))
            k.add_device(ptrs[1:], c[1:])
            for q in range(n_src):
                assert R.same_bits(k.read(q), ref[q])
            assert np.array_equal(k.plane_means(), ref_means)
            k.reset()
            k.finalize()
            assert all(np.all(k.read(q) == 0) for q in range(n_src))
        for p in ptrs:
            s.free(p)


@pytest.mark.gpu
def test_both_kernels_are_profiled():
    n, d = 16, 1e-4
    planes = R.noise_planes(np.random.default_rng(1), n, 2, d)
    with slicer_amd.Slicer(0) as s, slicer_amd.Rays(s, n, d) as rays:
        s.profile_enable(True)
        s.profile_reset()
        held = [DeviceMaps(s, maps) for maps in planes]
        rays.step(1.0, *held[0].ptrs)
        rays.step(2.0, *held[1].ptrs)
        rays.observe(3.0)
        prof = s.profile_get()
        s.profile_enable(False)
        for dm in held:
            dm.free()
    assert prof["rays_step"][0] == 2 and prof["rays_observe"][0] == 1


@pytest.mark.gpu
def test_create_refuses_with_a_handle_too():
    with slicer_amd.Slicer(0) as s:
        for npix, spacing, code in ((0, 1e-4, 2), (131073, 1e-4, 6), (16, 0.0, 2), (16, float("nan"), 2)):
            with pytest.raises(SlicerError) as e:
                slicer_amd.Rays(s, npix, spacing)
            assert e.value.code == code
