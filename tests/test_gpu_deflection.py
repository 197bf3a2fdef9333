"""Device deflection maps (slicer_shear_deflection) and finite-difference derivatives (slicer_fd_derivatives,
slicer_shear_fd) against the numpy restatement in tests/deflection_np.py."""
import math

import numpy as np
import pytest

import deflection_np as dn
import shear_np
import slicer_amd
from slicer_amd import lensing

ALPHAS = {"alpha1": slicer_amd.SHEAR_ALPHA1, "alpha2": slicer_amd.SHEAR_ALPHA2}
N6 = (slicer_amd.SHEAR_PHI, slicer_amd.SHEAR_GAMMA1, slicer_amd.SHEAR_GAMMA2, slicer_amd.SHEAR_GAMMA)
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 2, 3, 6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- spectral deflection ----

def kappa_inputs(n):
    rng = np.random.default_rng(n)
    return {"white": rng.standard_normal((n, n)).astype(np.float32), "clustered": shear_np.clustered(n, n + 1)}


def run_alpha(s, kappa, angle, split=False):
    """(N6 maps and spectrum read before deflection(), the same read after it, the two alpha maps)"""
    n = kappa.shape[0]
    s.set_option("shear_split", int(split))
    d = s.to_device(kappa)
    try:
        with slicer_amd.Shear(s, n, angle) as sh:
            sh.run(d)
            before = [sh.read(w) for w in N6] + [sh.spectrum()]
            sh.deflection()
            alpha = {k: sh.read(w) for k, w in ALPHAS.items()}
            after = [sh.read(w) for w in N6] + [sh.spectrum()]
            return before, after, alpha
    finally:
        s.free(d)
        s.set_option("shear_split", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", [(n, False) for n in (16, 30, 45, 49, 100, 1000)] + [(30, True), (45, True), (1024, True)])
def test_deflection_matches_restatement(n, split):
    angle = 5.0
    with slicer_amd.Slicer(0) as s:
        for label, kappa in kappa_inputs(n).items():
            ref = dict(zip(ALPHAS, dn.deflection(kappa, angle)))
            before, after, alpha = run_alpha(s, kappa, angle, split)
            for k in ALPHAS:
                ok, worst = shear_np.within_bound(alpha[k], ref[k])
                assert ok, f"{label} {k}: worst |d| / bound = {worst}"
            for a, b in zip(before, after):  # the maps of N6 and the spectrum are left as they were
                assert same(a, b)
            again = run_alpha(s, kappa, angle, split)[2]
            for k in ALPHAS:
                assert same(alpha[k], again[k]), k
            if split:
                plain = run_alpha(s, kappa, angle, False)[2]
                for k in ALPHAS:
                    assert same(alpha[k], plain[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,a,b", [(45, 7, 11), (45, -7, 11), (100, 13, 21), (100, -13, 21)])
def test_deflection_of_a_single_cosine(n, a, b):
    """Orientation and sign independent of numpy's FFT: kappa = A cos(x), x = 2 pi (a i0 + b i1) / n, has
    alpha_a = 2 A K_a sin(x) / k^2.  As in test_shear_of_a_single_cosine the device sees the cosine rounded to f32, so
    the reference is the closed form plus the restatement's answer for the rounding residual, under the map bound."""
    angle, A = 4.0, 0.7
    theta = np.deg2rad(angle)
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x = 2 * np.pi * ((a * i0 + b * i1) % n) / n
    kappa = A * np.cos(x)
    K0, K1 = 2 * np.pi * a / theta, 2 * np.pi * b / theta
    exact = {"alpha1": 2 * A * K0 * np.sin(x) / (K0 * K0 + K1 * K1), "alpha2": 2 * A * K1 * np.sin(x) / (K0 * K0 + K1 * K1)}
    k32 = kappa.astype(np.float32)
    res = dict(zip(ALPHAS, dn.deflection(k32.astype(np.float64) - kappa, angle)))
    with slicer_amd.Slicer(0) as s:
        alpha = run_alpha(s, k32, angle)[2]
    for k in ALPHAS:
        assert np.abs(res[k]).max() <= 1e-6 * np.abs(exact[k]).max()
        ok, worst = shear_np.within_bound(alpha[k], exact[k] + res[k])
        assert ok, (k, worst)


# ---- finite differences ----

T0, T1 = 16, 64  # the kernel's tile: rows x columns (slicer_fd.hip)
# 5 ... 13: below one tile, 11 and 13 on purpose (no restriction on the factors); around one tile side and two, a last
# tile of 4, 3, 2 and 1 samples (the one-sided D2 reaches 3 inward: a last tile of 1 or 2 takes them from the map)
FD_SIZES = sorted({5, 6, 7, 8, 9, 11, 13} | {t + k for t in (T0, T1) for k in (-1, 0, 1, 2, 3, 4)} | {2 * T0 + 1, 2 * T1 + 1}
                  | {1000, 4096})
FD_KINDS = ("white", "clustered", "one")


def phi_input(n, kind):
    if kind == "white":
        return np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
    if kind == "clustered":
        return shear_np.clustered(n, n + 1)
    return dn.noise_on_one(n, n + 2)


def spacings(n):
    return (1.0, math.radians(5.0) / n)


def run_fd(s, phi, d, which=tuple(range(slicer_amd.FD_COUNT)), shift_in=False, shift_out=False):
    """fd_derivatives, or the same through fd_run with the input / every output one float off the 16-byte grid"""
    n = phi.shape[0]
    if not shift_in and not shift_out:
        dp = s.to_device(phi)
        try:
            return slicer_amd.fd_derivatives(s, dp, n, d, which)
        finally:
            s.free(dp)
    pad = 1 if shift_in else 4  # floats in front of the map
    dp = s.to_device(np.concatenate([np.zeros(pad, np.float32), phi.ravel()]))
    bufs = {w: s.malloc(4 * (n * n + 1)) for w in which}
    off = 4 if shift_out else 0
    try:
        slicer_amd.fd_run(s, dp + 4 * pad, n, d, [bufs[w] + off if w in bufs else None for w in range(slicer_amd.FD_COUNT)])
        return {w: s.to_host(bufs[w] + off, (n, n), np.float32) for w in which}
    finally:
        s.free(dp)
        for p in bufs.values():
            s.free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FD_KINDS)
@pytest.mark.parametrize("n", FD_SIZES)
def test_fd_within_the_derived_bound(n, kind):
    phi = phi_input(n, kind)
    with slicer_amd.Slicer(0) as s:
        got = {d: dict(zip(dn.FD_NAMES, run_fd(s, phi, d).values())) for d in spacings(n)}
    for (d, k), worst in dn.fd_worst(phi, got, spacings(n)).items():
        assert worst <= 1.0, f"n = {n}, {kind}, d = {d}, {k}: worst |d| / bound = {worst}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [9, T0 + 1, T1 + 1])
def test_fd_of_polynomials_is_exact(n):
    """D2 of (i + j - c)^3 with d = 1 is 6 (i + j - c) and of (i + j - c)^2 with d = 2 is 1/2 everywhere, edges included,
    and every intermediate of the kernel is an exactly representable integer multiple: bit for bit."""
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    c = 3.0
    with slicer_amd.Slicer(0) as s:
        for f, d, kappa in (((i + j - c) ** 3, 1.0, 6 * (i + j - c)), ((i + j - c) ** 2, 2.0, np.full((n, n), 0.5))):
            phi = f.astype(np.float32)
            assert np.array_equal(phi.astype(np.float64), f)
            got = run_fd(s, phi, d, (slicer_amd.FD_KAPPA, slicer_amd.FD_GAMMA1))
            assert same(got[slicer_amd.FD_KAPPA], kappa.astype(np.float32))
            assert same(got[slicer_amd.FD_GAMMA1], np.zeros((n, n), np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, T1, T1 + 4, 1000])
def test_fd_is_the_same_wherever_the_pointers_lie_and_whatever_is_asked(n):
    """n = 64, 68, 1000 take the float4 stores when the outputs are aligned and the scalar ones when they are not."""
    phi = phi_input(n, "clustered")
    d = spacings(n)[1]
    with slicer_amd.Slicer(0) as s:
        full = run_fd(s, phi, d)
        for w in range(slicer_amd.FD_COUNT):
            assert same(run_fd(s, phi, d)[w], full[w])  # repeatable
        for kw in ({"shift_in": True}, {"shift_out": True}, {"shift_in": True, "shift_out": True}):
            moved = run_fd(s, phi, d, **kw)
            for w in range(slicer_amd.FD_COUNT):
                assert same(moved[w], full[w]), (kw, w)
        for w in range(slicer_amd.FD_COUNT):
            assert same(run_fd(s, phi, d, (w,))[w], full[w]), w


@pytest.mark.gpu
def test_shear_fd_equals_fd_derivatives_of_the_read_phi():
    n, angle = 49, 3.0
    kappa = shear_np.clustered(n, 3)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            with slicer_amd.Shear(s, n, angle) as sh:
                sh.run(d)
                sh.fd()
                got = [sh.read(slicer_amd.SHEAR_FD_ALPHA1 + w) for w in range(slicer_amd.FD_COUNT)]
                phi = sh.read(slicer_amd.SHEAR_PHI)
        finally:
            s.free(d)
        want = run_fd(s, phi, angle * math.pi / 180.0 / n)
        for w in range(slicer_amd.FD_COUNT):
            assert same(got[w], want[w]), w


def raises(code, call, text):
    with pytest.raises(slicer_amd.SlicerError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_fd_errors():
    n = 8
    with slicer_amd.Slicer(0) as s:
        dp, out = s.to_device(np.zeros((n, n), np.float32)), s.malloc(4 * n * n)
        try:
            ptrs = [out] + [None] * 5
            raises(ERR_ARG, lambda: lensing.fd_run(s, dp, 4, 1.0, ptrs), "npix = 4")
            for bad in (0.0, -1.0, float("inf"), float("nan")):
                raises(ERR_ARG, lambda: lensing.fd_run(s, dp, n, bad, ptrs), "spacing")
            raises(ERR_ARG, lambda: lensing.fd_run(s, None, n, 1.0, ptrs), "null")
            raises(ERR_ARG, lambda: lensing.fd_run(s, dp, n, 1.0, [None] * 6), "every output is null")
            raises(ERR_ARG, lambda: lensing.fd_run(s, dp, n, 1.0, [None, None, dp, None, None, None]), "output 2 is the input")
            lensing.fd_run(s, dp, n, 1.0, ptrs)
            assert np.all(s.to_host(out, (n, n), np.float32) == 0)
        finally:
            s.free(dp)
            s.free(out)


@pytest.mark.gpu
def test_deflection_and_fd_state():
    n = 16
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(shear_np.clustered(n, 1))
        try:
            with slicer_amd.Shear(s, n, 5.0) as sh:
                raises(ERR_STATE, sh.deflection, "before any slicer_shear_run")
                raises(ERR_STATE, sh.fd, "before any slicer_shear_run")
                sh.run(d)
                for w in (slicer_amd.SHEAR_ALPHA1, slicer_amd.SHEAR_ALPHA2):
                    raises(ERR_STATE, lambda: sh.read(w), "slicer_shear_deflection")
                    raises(ERR_STATE, lambda: sh.device_map(w), "slicer_shear_deflection")
                for w in range(slicer_amd.SHEAR_FD_ALPHA1, slicer_amd.SHEAR_FD_GAMMA + 1):
                    raises(ERR_STATE, lambda: sh.read(w), "slicer_shear_fd")
                for w in (4, 7, 10, 15, 22):
                    raises(ERR_ARG, lambda: sh.read(w), "which")
                sh.deflection()
                a1 = sh.read(slicer_amd.SHEAR_ALPHA1)
                raises(ERR_STATE, lambda: sh.read(slicer_amd.SHEAR_FD_KAPPA), "slicer_shear_fd")
                sh.fd()
                k = sh.read(slicer_amd.SHEAR_FD_KAPPA)
                sh.run(d)  # a new run: both sets are stale
                raises(ERR_STATE, lambda: sh.read(slicer_amd.SHEAR_ALPHA1), "slicer_shear_deflection")
                raises(ERR_STATE, lambda: sh.read(slicer_amd.SHEAR_FD_KAPPA), "slicer_shear_fd")
                sh.deflection()
                sh.fd()
                assert same(sh.read(slicer_amd.SHEAR_ALPHA1), a1) and same(sh.read(slicer_amd.SHEAR_FD_KAPPA), k)
            with slicer_amd.Shear(s, 4, 5.0) as sh:
                sh.run(d)
                raises(ERR_UNSUPPORTED, sh.fd, "npix = 4")
                sh.deflection()
                assert sh.read(slicer_amd.SHEAR_ALPHA2).shape == (4, 4)
        finally:
            s.free(d)
