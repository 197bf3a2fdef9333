"""SLICER_amd --kappa ... --power: the power-spectrum file written by the driver against the numpy
restatement (tests/power_np.py) applied to the kappa files of the same run."""
import os

import numpy as np
import pytest

import power_np
import slicer_amd
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

ANGLE = 2.0  # make_cone's field of view


def cl_file(out, npix):
    return os.path.join(out, f"cone_gadget.cl_{npix}_t0.txt")


def parse(path):
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    meta = {h[0]: h[1:] for h in head[:3]}
    table = np.loadtxt(path, ndmin=2)
    return meta, head[3], table


def kappa_maps(out, zs, npix):
    names = os.listdir(out)
    maps = []
    for z in zs:
        name = [f for f in names if f.startswith(f"cone_gadget.kappa_z{z:.4f}_")]
        assert len(name) == 1, (z, name)
        maps.append(read_fits(os.path.join(out, name[0]), npix)[1])
    return maps


def check_against_kappa_files(out, npix, cross, edges=None):
    meta, cols, table = parse(cl_file(out, npix))
    assert meta["npix"] == [str(npix)] and float(meta["angle_deg"][0]) == ANGLE
    zs = [float(z) for z in meta["zs"]]
    S = len(zs)
    pairs = power_np.pairs(S, cross)
    assert cols == ["ell_lo", "ell_hi", "ell_mean", "n_modes"] + [f"C_{s}_{t}" for s, t in pairs]
    edges = power_np.default_edges(npix) if edges is None else np.asarray(edges, np.float64)
    B = edges.size - 1
    assert table.shape == (B, 4 + len(pairs))
    ell_f = slicer_amd.ell_fundamental(ANGLE)
    assert np.array_equal(table[:, 0], edges[:-1] * ell_f) and np.array_equal(table[:, 1], edges[1:] * ell_f)
    bins = slicer_amd.power_bins(npix, edges)
    assert np.array_equal(table[:, 3].astype(np.int64), bins["counts"])
    assert np.array_equal(table[:, 2], bins["mean_radius"] * ell_f, equal_nan=True)
    maps = kappa_maps(out, zs, npix)
    exact = [np.fft.rfft2(m.astype(np.float64)) for m in maps]
    ref = power_np.power_of_spectra(exact, ANGLE, edges, cross=True)
    nz = ref["counts"] > 0
    eps = [1e-12 * np.log2(npix) * np.linalg.norm(m.astype(np.float64)) for m in maps]
    counts, mags = power_np.binned_sums(npix, edges, [np.abs(x) for x in exact])
    norm = np.radians(ANGLE) ** 2 / float(npix) ** 4
    for q, (s, t) in enumerate(pairs):
        got = table[:, 4 + q]
        assert np.array_equal(np.isnan(got), ~nz)
        ms, mt = mags[s][nz] / counts[nz], mags[t][nz] / counts[nz]
        bnd = norm * (eps[s] * mt + eps[t] * ms + eps[s] * eps[t]) + 1e-13 * np.abs(ref["cl"][s, t][nz])
        assert np.all(np.abs(got[nz] - ref["cl"][s, t][nz]) <= bnd), (s, t)
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [32, 30])
def test_power_file_matches_the_restatement_of_the_kappa_files(tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini, "--ngp", "--kappa", "all", "--shear", "--power", "auto"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, cross=False) >= 20
    with_power = {k: files(out, k) for k in (".kappa_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".phi_z", ".plane_")}
    os.remove(cl_file(out, npix))
    clear(out)
    r = run([ini, "--ngp", "--kappa", "0.05,0.1,0.2", "--power", "cross"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, cross=True) == 3
    # kappa, shear and plane files are byte-identical with and without --power, and no spectrum file appears
    os.remove(cl_file(out, npix))
    clear(out)
    r = run([ini, "--ngp", "--kappa", "all", "--shear"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: files(out, k) for k in with_power} == with_power
    assert not files(out, ".cl_")


@pytest.mark.gpu
def test_power_file_of_every_pair_of_every_plane(tmp_path):
    """--kappa all makes one source per plane: more than 8, so the binning runs over pairs of source blocks."""
    ini, _, out = make_cone(tmp_path)
    r = run([ini, "--ngp", "--kappa", "all", "--power", "cross"])
    assert r.returncode == 0, r.stderr[-2000:]
    S = check_against_kappa_files(out, 32, cross=True)
    assert S >= 20
    _, cols, table = parse(cl_file(out, 32))
    assert len(cols) - 4 == table.shape[1] - 4 == S * (S + 1) // 2 >= 210


@pytest.mark.gpu
def test_power_file_is_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.2", "--power", "cross"]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = open(cl_file(out, 32), "rb").read()
    # resume: some plane files removed, the others read back; the kappa files go first (they are not overwritten),
    # the spectrum file is left in place and rewritten
    for f in files(out, ".kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    with open(cl_file(out, 32), "w") as f:
        f.write("stale\n")
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert open(cl_file(out, 32), "rb").read() == one
    clear(out)
    os.remove(cl_file(out, 32))
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(cl_file(out, 32), "rb").read() == one


@pytest.mark.gpu
def test_power_edges_are_honoured(tmp_path):
    ini, _, out = make_cone(tmp_path)
    edges = [0.5, 2.0, 5.0, 9.5, 40.0]
    r = run([ini, "--ngp", "--kappa", "0.1,0.2", "--power", "auto", "--power-edges", ",".join(map(str, edges))])
    assert r.returncode == 0, r.stderr[-2000:]
    check_against_kappa_files(out, 32, cross=False, edges=edges)


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args", [
    (32, ["--power", "auto"]),
    (37, ["--kappa", "all", "--power", "auto"]),
    (32, ["--kappa", "all", "--power", "both"]),
    (32, ["--kappa", "all", "--power", "auto", "--power-edges", "3,1"]),
    (32, ["--kappa", "all", "--power", "auto", "--power-edges", "0,x"]),
    (32, ["--kappa", "all", "--power-edges", "0,1"]),
    (32, ["--kappa", ",".join(f"{0.01 + 0.001 * i:.3f}" for i in range(129)), "--power", "cross"]),
])
def test_power_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "power" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".cl_" in f]
