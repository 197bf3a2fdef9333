"""SLICER_amd --kappa: Born convergence maps written by the driver against the numpy
restatement (tests/kappa_np.py) applied to the plane files and planes_list of the same run."""
import os

import numpy as np
import pytest

import kappa_np
from test_driver import make_cone, run


def read_fits(path, npix=32):
    raw = open(path, "rb").read()
    hdr = raw[:2880]
    return hdr, np.frombuffer(raw[2880:2880 + 4 * npix * npix], ">f4").reshape(npix, npix).astype(np.float32)


def card_value(hdr, key):
    for i in range(0, 2880, 80):
        c = hdr[i:i + 80].decode()
        if c.startswith(key.ljust(8) + "="):
            return float(c[10:].split("/")[0])
    raise KeyError(key)


def files(out, what):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if what in f}


@pytest.mark.gpu
def test_kappa_all_matches_the_restatement_and_leaves_the_planes_alone(tmp_path):
    ini, _, out = make_cone(tmp_path)
    r = run([ini, "--ngp", "--kappa", "all"])   # (NGP: bitwise reproducible planes, see below)
    assert r.returncode == 0, r.stderr[-2000:]
    planes = sorted(f for f in os.listdir(out) if ".plane_32_t0.fits" in f)
    P = len(planes)
    assert P >= 20
    rows = [ln.split() for ln in open(os.path.join(out, "cone_planes_list_t0.txt")).read().strip().split("\n")]
    ld = np.array([float(r[2]) for r in rows])
    ld2 = np.array([float(r[3]) for r in rows])
    zsnap = np.array([float(r[6]) for r in rows])
    maps = []
    for f in planes:
        hdr, m = read_fits(os.path.join(out, f))
        assert card_value(hdr, "DLLOW") * 0.7 == pytest.approx(ld[len(maps)], rel=1e-5)
        maps.append(m)
    c, zlo, zup, zl, chil = kappa_np.weights(0.3, -1.0, 2.0, 32, ld, ld2, zsnap)
    ref = kappa_np.kappa(maps, c)
    kap = files(out, ".kappa_z")
    assert len(kap) == P
    live = 0
    for s in range(P):
        name = "cone_gadget.kappa_z%.4f_32_t0.fits" % zup[s]
        hdr, m = read_fits(os.path.join(out, name))
        assert card_value(hdr, "ZSOURCE") == pytest.approx(zup[s], rel=1e-9)
        assert card_value(hdr, "ANGLE") == 2.0
        # (the planes_list columns carry 6 digits: the weights agree to ~1e-6 relative, not to the last bit)
        bound = 2e-6 * np.abs(ref[s]) + 1e-6 * np.abs(ref[s]).max()
        assert np.all(np.abs(m - ref[s]) <= bound), (s, float(np.max(np.abs(m - ref[s]) - bound)))
        live += int(np.abs(m).max() > 0)   # (the nearest planes of a 2-degree cone may hold no particle)
    assert live >= P - 4
    # the plane files are byte-identical to those of a run without --kappa
    with_kappa = files(out, ".plane_")
    for f in os.listdir(out):
        if f.endswith(".fits"):
            os.remove(os.path.join(out, f))
    assert run([ini, "--ngp"]).returncode == 0
    assert files(out, ".plane_") == with_kappa
    assert not files(out, ".kappa_z")


@pytest.mark.gpu
def test_resumed_and_two_rank_runs_give_the_same_kappa(tmp_path):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.1,0.2", "--kappa-no-growth"]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = files(out, ".kappa_z")
    assert sorted(one) == ["cone_gadget.kappa_z0.0500_32_t0.fits", "cone_gadget.kappa_z0.1000_32_t0.fits",
                           "cone_gadget.kappa_z0.2000_32_t0.fits"]
    # resume: every plane file is left in place and read back; some of them removed, so that passes mix both
    for f in one:
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert files(out, ".kappa_z") == one
    for f in one:
        os.remove(os.path.join(out, f))
    r = run([ini] + args)   # every plane skipped
    assert r.returncode == 0 and r.stdout.count("Already exists") == len(planes)
    assert files(out, ".kappa_z") == one
    # two ranks on one GPU, summed through host memory in fixed point: byte-identical
    for f in os.listdir(out):
        if f.endswith(".fits"):
            os.remove(os.path.join(out, f))
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, ".kappa_z") == one
