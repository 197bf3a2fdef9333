"""SLICER_amd --kappa ... --moments: the moments file written by the driver against the numpy
restatement (tests/moments_np.py) applied to the kappa files of the same run."""
import os

import numpy as np
import pytest

import moments_np as M
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

ANGLE = 2.0  # make_cone's field of view
LD = np.longdouble


def moments_file(out, npix):
    return os.path.join(out, f"cone_gadget.moments_{npix}_t0.txt")


def check_against_kappa_files(out, npix, levels):
    path = moments_file(out, npix)
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    assert head[0] == ["npix", str(npix)] and head[1][0] == "angle_deg" and float(head[1][1]) == ANGLE
    assert head[2] == ["levels", str(levels)]
    assert head[3] == ["z", "level", "npix", "mean"] + [f"S{k}" for k in M.ORDERS]
    table = np.loadtxt(path, ndmin=2)
    assert table.shape[1] == 11 and table.shape[0] % (levels + 1) == 0
    S = table.shape[0] // (levels + 1)
    names = os.listdir(out)
    for s in range(S):
        rows = table[s * (levels + 1):(s + 1) * (levels + 1)]
        z = rows[0, 0]
        name = [f for f in names if f.startswith(f"cone_gadget.kappa_z{z:.4f}_")]
        assert len(name) == 1, (z, name)
        pyr = M.pyramid(read_fits(os.path.join(out, name[0]), npix)[1], levels, "mean")
        for l, x in enumerate(pyr):
            n = x.shape[0]
            assert rows[l, 0] == z and rows[l, 1] == l and rows[l, 2] == n == npix >> l
            mean, mean_abs = M.mean_ld(x)
            assert abs(LD(rows[l, 3]) - mean) <= M.mean_bound(mean_abs, n), (s, l)
            ref, A = M.sums_ld(x, rows[l, 3])  # the centre is the level's own mean, as printed (%.17g round-trips)
            assert np.all(np.abs(rows[l, 4:].astype(LD) - ref) <= M.sum_bounds(A, n)), (s, l)
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix,levels", [(32, 5), (30, 4), (37, 0)])
def test_moments_file_matches_the_restatement_of_the_kappa_files(tmp_path, npix, levels):
    ini, _, out = make_cone(tmp_path, npix=npix)
    shear = ["--shear", "--power", "auto"] if npix != 37 else []  # (37 is not a size the transforms take)
    args = [ini, "--ngp", "--kappa", "all"] + shear
    r = run(args + ["--moments"] + (["--moments-levels", str(levels)] if levels else []))
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, levels) >= 20
    kinds = (".kappa_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".phi_z", ".plane_", ".cl_")
    with_moments = {k: files(out, k) for k in kinds}
    assert len(with_moments[".cl_"]) == (1 if shear else 0)
    # plane, kappa, shear and spectrum files are byte-identical without --moments, and no moments file appears
    os.remove(moments_file(out, npix))
    clear(out)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: files(out, k) for k in kinds} == with_moments
    assert not files(out, ".moments_")


@pytest.mark.gpu
def test_moments_file_is_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "3"]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, 32, 3) == 2
    one = open(moments_file(out, 32), "rb").read()
    # resume: some plane files removed, the others read back; the moments file is left in place and rewritten
    for f in files(out, ".kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    with open(moments_file(out, 32), "w") as f:
        f.write("stale\n")
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert open(moments_file(out, 32), "rb").read() == one
    clear(out)
    os.remove(moments_file(out, 32))
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(moments_file(out, 32), "rb").read() == one


@pytest.mark.gpu
@pytest.mark.parametrize("args", [
    ["--moments"],
    ["--kappa", "all", "--moments-levels", "2"],
    ["--kappa", "all", "--moments", "--moments-levels", "6"],
    ["--kappa", "all", "--moments", "--moments-levels", "-1"],
    ["--kappa", "all", "--moments", "--moments-levels", "two"],
    ["--kappa", "all", "--moments", "--moments-levels"],
])
def test_moments_are_refused_before_any_plane(tmp_path, args):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "moments" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".moments_" in f or ".cl_" in f]
