"""Device shear and lensing-potential maps (slicer_shear_*, slicer_amd.Shear) against the f64
numpy restatement in tests/shear_np.py."""
import numpy as np
import pytest

import shear_np
import slicer_amd

WHICH = {"phi": slicer_amd.SHEAR_PHI, "gamma1": slicer_amd.SHEAR_GAMMA1, "gamma2": slicer_amd.SHEAR_GAMMA2,
         "gamma": slicer_amd.SHEAR_GAMMA}


def inputs(n):
    rng = np.random.default_rng(n)
    return {"white": rng.standard_normal((n, n)).astype(np.float32), "clustered": shear_np.clustered(n, n + 1)}


def run_maps(s, kappa, angle, names=tuple(WHICH), split=False):
    n = kappa.shape[0]
    s.set_option("shear_split", int(split))
    d = s.to_device(kappa)
    try:
        with slicer_amd.Shear(s, n, angle) as sh:
            sh.run(d)
            return sh.spectrum(), {k: sh.read(WHICH[k]) for k in names}
    finally:
        s.free(d)
        s.set_option("shear_split", 0)


def check_spectrum(got, ref, kappa):
    n = kappa.shape[0]
    bound = 1e-12 * np.log2(n) * np.linalg.norm(kappa.astype(np.float64))
    err = float(np.abs(got - ref).max())
    assert err <= bound, (err, bound)


def check_map(name, got, ref):
    ok, worst = shear_np.within_bound(got, ref)
    assert ok, f"{name}: worst |d| / bound = {worst}"


CASES = [(n, False) for n in (16, 30, 45, 49, 100, 1000, 4000, 4096)] + [(1024, True), (30, True), (45, True)]


def check_size(n, split):
    """Spectrum and the four maps of a white-noise and a clustered map against the restatement; a second run bitwise."""
    angle = 5.0 if n < 1000 else 10.0
    with slicer_amd.Slicer(0) as s:
        for label, kappa in inputs(n).items():
            ref = shear_np.shear(kappa, angle)
            spec, maps = run_maps(s, kappa, angle, split=split)
            check_spectrum(spec, ref["spectrum"], kappa)
            for k in WHICH:
                check_map(f"{label} {k}", maps[k], ref[k])
            spec2, maps2 = run_maps(s, kappa, angle, split=split)
            assert np.array_equal(spec.view(np.uint64), spec2.view(np.uint64))
            for k in WHICH:
                assert np.array_equal(maps[k].view(np.uint32), maps2[k].view(np.uint32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_shear_matches_restatement(n, split):
    check_size(n, split)


# Every supported size up to 1200, unforced.  The plan is not exported, so what the sizes reach is restated here from
# plan_chain (slicer_fft.hip): 2 ... 15 are single-stage and stage-less plans (n = 2: a row chain of length 1);
# up to 1024 the columns take one pass, from 1029 on two, and the second pass's radix runs through 2, 3, 5, 7 and their
# products (1029 = 343 * 3, 1050 = 525 * 2, 1080 = 540 * 2, 1125 = 375 * 3, 1134 = 567 * 2, 1176 = 588 * 2, 1200 = 600 * 2, ...),
# odd n (packed row pairs, a missing last row) included.
SWEEP = [n for n in range(2, 1201) if shear_np.seven_smooth(n)]
# The same with shear_split = 1 (radix at most sqrt(L), or the smallest prime factor: chains of up to four passes).
SWEEP_SPLIT = [n for n in SWEEP if n <= 200]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWEEP)
def test_shear_sweep(n):
    check_size(n, False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SWEEP_SPLIT)
def test_shear_sweep_forced_split(n):
    check_size(n, True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4802, 8505])
def test_shear_two_pass_representatives(n):
    """4802 = 2 7^4: rows 2401, columns 686 * 7.  8505 = 3^5 5 7: the smallest size whose rows take two passes (odd n
    above 8192: the packed-pair loads and stores around a two-pass row chain), rows 2835 * 3, columns 945 * (3, 3)."""
    check_size(n, False)


def check_large(n, seed, names):
    """One clustered map at a size whose host reference needs gigabytes: the spectrum, then one filtered inverse at a
    time."""
    angle = 10.0
    kappa = shear_np.clustered(n, seed)
    with slicer_amd.Slicer(0) as s:
        spec, maps = run_maps(s, kappa, angle, names=names)
    khat = np.fft.rfft2(kappa.astype(np.float64))
    check_spectrum(spec, khat, kappa)
    del spec
    ref = {}
    for k, which in (("gamma1", 1), ("gamma2", 2)):
        if k in names:
            f = shear_np.filters(n, angle)[which]
            ref[k] = np.fft.irfft2(khat * f, s=(n, n))
            del f
            check_map(k, maps[k], ref[k])
    if "gamma" in names:
        check_map("gamma", maps["gamma"], np.sqrt(ref["gamma1"] ** 2 + ref["gamma2"] ** 2))


@pytest.mark.gpu
def test_shear_16384_gamma1_and_spectrum():
    check_large(16384, 7, ("gamma1",))


@pytest.mark.gpu
@pytest.mark.parametrize("n,names", [
    (12005, ("gamma1", "gamma2", "gamma")),   # 5 7^4, odd: rows 2401 * 5, three lines of 7^4 per workgroup; columns 343 * (5, 7)
    (15625, ("gamma1", "gamma2", "gamma")),   # 5^6, the largest odd size: rows 3125 * 5, columns 625 * 25
    (14406, ("gamma1",)),                     # 2 3 7^4: row radix 7203 = 3 7^4, one line per workgroup; columns 686 * (3, 7)
    (16200, ("gamma1",)),                     # 2^3 3^4 5^2: row radix 8100, one line per workgroup; columns 900 * (2, 3, 3)
])
def test_shear_large_plan_classes(n, names):
    """The odd sizes read gamma2 and |gamma| as well: the packed-pair store of gamma1, gamma2 and |gamma| is the last
    pass of the gamma2 chain only."""
    check_large(n, n % 1000, names)


def cosine_case(n, a, b, angle=4.0, A=0.7):
    """kappa = A cos(2 pi (a i0 + b i1) / n), 0 <= b < n / 2, 0 < |a| < n / 2, and what the contract makes of it by
    hand: khat = A n^2 / 2 at (a mod n, b) (and at (-a mod n, 0) when b = 0), phi, gamma1, gamma2 the same cosine times
    the filter value at (a, b)."""
    theta = np.deg2rad(angle)
    i0, i1 = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    kappa = A * np.cos(2 * np.pi * ((a * i0 + b * i1) % n) / n)
    del i0, i1
    k2 = float(a * a + b * b)
    spec = np.zeros((n, n // 2 + 1), np.complex128)
    spec[a % n, b] = A * n * n / 2
    if b == 0:
        spec[-a % n, 0] = A * n * n / 2
    return kappa, {"spectrum": spec, "phi": -2.0 / ((2 * np.pi / theta) ** 2 * k2) * kappa,
                   "gamma1": (a * a - b * b) / k2 * kappa, "gamma2": 2.0 * a * b / k2 * kappa}


# two column passes at both sizes; 8505 has two row passes as well.  Modes: both signs of the row frequency, and b = 0
# (two coefficients in the half plane, gamma2 = 0).
COSINES = [(2058, 296, 412), (2058, -296, 412), (2058, 687, 0), (1125, 162, 226), (1125, -162, 226), (1125, 376, 0),
           (8505, -1217, 1702)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,a,b", COSINES)
def test_shear_of_a_single_cosine(n, a, b):
    """Orientation and sign independent of numpy's FFT.  The device sees the cosine rounded to f32; the transform is
    linear, so the reference is the analytic answer for the exact cosine plus the restatement's answer for the rounding
    residual (2^-24 of the field: numpy's conventions enter at that level only)."""
    angle = 4.0
    kappa, exact = cosine_case(n, a, b, angle)
    k32 = kappa.astype(np.float32)
    res = shear_np.shear(k32.astype(np.float64) - kappa, angle)
    assert np.abs(res["gamma1"]).max() <= 1e-6 * np.abs(kappa).max()
    ref = {k: exact[k] + res[k] for k in exact}
    ref["gamma"] = np.sqrt(ref["gamma1"] ** 2 + ref["gamma2"] ** 2)
    del exact, res
    with slicer_amd.Slicer(0) as s:
        spec, maps = run_maps(s, k32, angle)
    check_spectrum(spec, ref["spectrum"], k32)
    for k in WHICH:
        if k == "gamma2" and b == 0:
            # gamma2 of this field is 0 (only the f32 residual's is left), so the absolute floor of the map bound,
            # 1e-9 of the map's size, has nothing to scale with: it is taken from gamma1 of the same field, which goes
            # through the same chain of passes with the same magnitudes.
            assert np.abs(maps[k] - ref[k]).max() <= 1e-9 * np.abs(ref["gamma1"]).max()
        else:
            check_map(k, maps[k], ref[k])


@pytest.mark.gpu
def test_shear_errors():
    with slicer_amd.Slicer(0) as s:
        for n in (37, 44, 0, 1, 16385):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Shear(s, n, 5.0)
            assert e.value.code == 6, n  # SLICER_ERR_UNSUPPORTED
        for angle in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Shear(s, 16, angle)
            assert e.value.code == 2, angle  # SLICER_ERR_ARG
        with slicer_amd.Shear(s, 16, 5.0) as sh:
            for call in (lambda: sh.read(0), lambda: sh.spectrum(), lambda: sh.device_map(3)):
                with pytest.raises(slicer_amd.SlicerError) as e:
                    call()
                assert e.value.code == 3  # SLICER_ERR_STATE: nothing has run
            with pytest.raises(slicer_amd.SlicerError) as e:
                sh.run(0)
            assert e.value.code == 2
            d = s.to_device(np.zeros((16, 16), np.float32))
            try:
                sh.run(d)
                for which in (-1, 4):
                    with pytest.raises(slicer_amd.SlicerError) as e:
                        sh.read(which)
                    assert e.value.code == 2
                assert np.all(sh.read(slicer_amd.SHEAR_GAMMA) == 0)
            finally:
                s.free(d)


@pytest.mark.gpu
def test_run_kappa_equals_run_on_the_read_map():
    n, angle = 64, 3.0
    rng = np.random.default_rng(5)
    maps = (rng.gamma(0.5, 2.0, (3, n, n)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-4, 1e-3, (2, 3))
    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(m) for m in maps]
        try:
            with slicer_amd.Kappa(s, n, 2) as k, slicer_amd.Shear(s, n, angle) as sh:
                k.add_device(ptrs, coeff.T)
                k.finalize()
                sh.run_kappa(k, 1)
                a = {w: sh.read(w) for w in WHICH.values()}
                spec_a = sh.spectrum()
                d = s.to_device(k.read(1))
                try:
                    sh.run(d)
                    for w in WHICH.values():
                        assert np.array_equal(a[w].view(np.uint32), sh.read(w).view(np.uint32))
                    assert np.array_equal(spec_a.view(np.uint64), sh.spectrum().view(np.uint64))
                finally:
                    s.free(d)
        finally:
            for p in ptrs:
                s.free(p)
