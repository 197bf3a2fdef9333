"""SLICER_amd --kappa ... --shear: shear and lensing-potential maps written by the driver against
the numpy restatement (tests/shear_np.py) applied to the kappa files of the same run."""
import os

import numpy as np
import pytest

import shear_np
from test_driver import make_cone, run

OUTS = {".gamma1_z": "gamma1", ".gamma2_z": "gamma2", ".gamma_z": "gamma", ".phi_z": "phi"}


def read_fits(path, npix):
    raw = open(path, "rb").read()
    return raw[:2880], np.frombuffer(raw[2880:2880 + 4 * npix * npix], ">f4").reshape(npix, npix).astype(np.float32)


def files(out, what):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if what in f}


def clear(out):
    for f in os.listdir(out):
        if f.endswith(".fits"):
            os.remove(os.path.join(out, f))


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [32, 30])
def test_shear_files_match_the_restatement_of_the_kappa_files(tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini, "--ngp", "--kappa", "all", "--shear"])
    assert r.returncode == 0, r.stderr[-2000:]
    kap = files(out, ".kappa_z")
    assert len(kap) >= 20
    for name in kap:
        hdr, k = read_fits(os.path.join(out, name), npix)
        ref = shear_np.shear(k, 2.0)
        for token, what in OUTS.items():
            sname = name.replace(".kappa_z", token)
            shdr, m = read_fits(os.path.join(out, sname), npix)
            assert shdr == hdr, sname
            ok, worst = shear_np.within_bound(m, ref[what])
            assert ok, (sname, worst)
    shear_files = {t: files(out, t) for t in OUTS}
    assert all(len(v) == len(kap) for v in shear_files.values())
    # the kappa and plane files are byte-identical to those of a run without --shear
    planes = files(out, ".plane_")
    clear(out)
    r = run([ini, "--ngp", "--kappa", "all"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, ".kappa_z") == kap
    assert files(out, ".plane_") == planes
    for t in OUTS:
        assert not files(out, t)


@pytest.mark.gpu
def test_two_rank_run_gives_the_same_shear_files(tmp_path):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.2", "--shear"]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = {t: files(out, t) for t in OUTS}
    assert sorted(one[".gamma1_z"]) == ["cone_gadget.gamma1_z0.0500_32_t0.fits", "cone_gadget.gamma1_z0.2000_32_t0.fits"]
    clear(out)
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert {t: files(out, t) for t in OUTS} == one


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args", [(32, ["--shear"]), (37, ["--kappa", "all", "--shear"])])
def test_shear_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "shear" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits")]
