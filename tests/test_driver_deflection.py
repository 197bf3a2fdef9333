"""SLICER_amd --kappa ... --shear --deflection [--shear-derivative fft|gradient]: the deflection files and the
finite-difference shear files written by the driver against the numpy restatement
(tests/deflection_np.py) applied to the kappa and phi files of the same run."""
import math
import os

import numpy as np
import pytest

import deflection_np as dn
import shear_np
import slicer_amd
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

ANGLE = 2.0  # make_cone's fov
ALPHA = {".alpha1_z": "alpha1", ".alpha2_z": "alpha2"}
GAMMA = {".gamma1_z": "gamma1", ".gamma2_z": "gamma2", ".gamma_z": "gamma"}
EVERY = (".plane_", ".kappa_z", ".phi_z") + tuple(GAMMA) + tuple(ALPHA)


def snapshot(out):
    return {t: files(out, t) for t in EVERY}


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [32, 30])
def test_fft_deflection_files_match_the_restatement_of_the_kappa_files(tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini, "--ngp", "--kappa", "all", "--shear", "--deflection"])
    assert r.returncode == 0, r.stderr[-2000:]
    with_alpha = snapshot(out)
    kap = with_alpha[".kappa_z"]
    assert len(kap) >= 20
    for name in kap:
        hdr, k = read_fits(os.path.join(out, name), npix)
        ref = dict(zip(("alpha1", "alpha2"), dn.deflection(k, ANGLE)))
        for token, what in ALPHA.items():
            aname = name.replace(".kappa_z", token)
            ahdr, m = read_fits(os.path.join(out, aname), npix)
            assert ahdr == hdr, aname
            ok, worst = shear_np.within_bound(m, ref[what])
            assert ok, (aname, worst)
    assert all(len(with_alpha[t]) == len(kap) for t in ALPHA)
    # plane, kappa, phi and gamma files are byte-identical to those of a run without --deflection; an explicit
    # --shear-derivative fft is the default
    for extra in ([], ["--shear-derivative", "fft", "--deflection"]):
        clear(out)
        r = run([ini, "--ngp", "--kappa", "all", "--shear"] + extra)
        assert r.returncode == 0, r.stderr[-2000:]
        now = snapshot(out)
        for t in EVERY:
            assert now[t] == (with_alpha[t] if extra or t not in ALPHA else {}), (extra, t)


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [32, 30])
def test_gradient_files_are_the_finite_differences_of_the_phi_file(tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini, "--ngp", "--kappa", "0.05,0.2", "--shear", "--deflection"])
    assert r.returncode == 0, r.stderr[-2000:]
    fft = snapshot(out)
    clear(out)
    r = run([ini, "--ngp", "--kappa", "0.05,0.2", "--shear", "--deflection", "--shear-derivative", "gradient"])
    assert r.returncode == 0, r.stderr[-2000:]
    grad = snapshot(out)
    for t in (".plane_", ".kappa_z", ".phi_z"):  # unchanged by the choice of derivative
        assert grad[t] == fft[t] and grad[t], t
    d = ANGLE * math.pi / 180.0 / npix
    with slicer_amd.Slicer(0) as s:
        for name in grad[".phi_z"]:
            hdr, phi = read_fits(os.path.join(out, name), npix)
            dp = s.to_device(phi)
            try:
                dev = dict(zip(dn.FD_NAMES, slicer_amd.fd_derivatives(s, dp, npix, d).values()))
            finally:
                s.free(dp)
            got = {}
            for token, what in {**GAMMA, **ALPHA}.items():
                fname = name.replace(".phi_z", token)
                fhdr, got[what] = read_fits(os.path.join(out, fname), npix)
                assert fhdr == hdr, fname
                assert np.array_equal(got[what].view(np.uint32), dev[what].view(np.uint32)), fname
                assert grad[token][fname] != fft[token][fname]  # and not the FFT maps under another name
            got["kappa"] = dev["kappa"]
            for (_, k), worst in dn.fd_worst(phi, {d: got}, (d,)).items():
                assert worst <= 1.0, (name, k, worst)
    clear(out)  # without --deflection: the same gamma files, no alpha files
    r = run([ini, "--ngp", "--kappa", "0.05,0.2", "--shear", "--shear-derivative", "gradient"])
    assert r.returncode == 0, r.stderr[-2000:]
    now = snapshot(out)
    for t in EVERY:
        assert now[t] == ({} if t in ALPHA else grad[t]), t


@pytest.mark.gpu
@pytest.mark.parametrize("derivative", ["fft", "gradient"])
def test_two_rank_run_gives_the_same_files(tmp_path, derivative):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.2", "--shear", "--deflection", "--shear-derivative", derivative]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = snapshot(out)
    assert sorted(one[".alpha1_z"]) == ["cone_gadget.alpha1_z0.0500_32_t0.fits", "cone_gadget.alpha1_z0.2000_32_t0.fits"]
    clear(out)
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert snapshot(out) == one


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args,text", [
    (32, ["--kappa", "all", "--deflection"], "--deflection needs --shear"),
    (32, ["--kappa", "all", "--shear-derivative", "gradient"], "--shear-derivative needs --shear"),
    (32, ["--kappa", "all", "--shear", "--shear-derivative", "stencil"], "bad --shear-derivative"),
    (4, ["--kappa", "all", "--shear", "--shear-derivative", "gradient"], "npix = 4"),
])
def test_bad_requests_are_refused_before_any_plane(tmp_path, npix, args, text):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert text in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits")]
