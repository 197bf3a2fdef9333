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


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_shear_matches_restatement(n, split):
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
def test_shear_16384_gamma1_and_spectrum():
    n, angle = 16384, 10.0
    kappa = shear_np.clustered(n, 7)
    with slicer_amd.Slicer(0) as s:
        spec, maps = run_maps(s, kappa, angle, names=("gamma1",))
    khat = np.fft.rfft2(kappa.astype(np.float64))
    check_spectrum(spec, khat, kappa)
    del spec
    _, fg1, _ = shear_np.filters(n, angle)
    khat *= fg1
    del fg1
    check_map("gamma1", maps["gamma1"], np.fft.irfft2(khat, s=(n, n)))


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
