"""SLICER_amd --kappa ... --bispectrum: the bispectrum file written by the driver against the numpy
restatement (tests/bispectrum_np.py) applied to the kappa files of the same run."""
import os

import numpy as np
import pytest

import bispectrum_np
import slicer_amd
from test_driver import make_cone, run
from test_driver_power import ANGLE, kappa_maps
from test_driver_shear import clear, files

EDGES = [0.0, 1.5, 3.0, 4.5, 6.5, 9.0, 12.0]


def bl_file(out, npix):
    return os.path.join(out, f"cone_gadget.bl_{npix}_t0.txt")


def parse(path):
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    meta = {h[0]: h[1:] for h in head[:4]}
    table = np.loadtxt(path, ndmin=2)
    return meta, head[4], table


def check_against_kappa_files(out, npix, kind, edges):
    meta, cols, table = parse(bl_file(out, npix))
    assert list(meta) == ["npix", "angle_deg", "zs", "ell_edges"]
    assert meta["npix"] == [str(npix)] and float(meta["angle_deg"][0]) == ANGLE
    zs = [float(z) for z in meta["zs"]]
    S = len(zs)
    edges = np.asarray(edges, np.float64)
    B = edges.size - 1
    ell_f = slicer_amd.ell_fundamental(ANGLE)
    assert np.array_equal(np.array([float(x) for x in meta["ell_edges"]]), edges * ell_f)
    assert cols == ["i", "j", "k", "ell_mean_i", "ell_mean_j", "ell_mean_k", "n_triangles"] + [f"B_{s}" for s in range(S)]
    tr = slicer_amd.bispectrum_triples(B, kind)
    assert table.shape == (tr.shape[0], 7 + S)
    assert np.array_equal(table[:, :3].astype(np.int32), tr)
    mean = slicer_amd.power_bins(npix, edges)["mean_radius"] * ell_f
    for c in range(3):
        assert np.array_equal(table[:, 3 + c], mean[tr[:, c]], equal_nan=True)
    exact = slicer_amd.bispectrum_triangles(npix, edges, tr)
    assert np.array_equal(table[:, 6].astype(np.int64), exact)
    # every B_s within bound (f) of tests/test_gpu_bispectrum.py of the restatement of the run's own kappa file
    N = bispectrum_np.full_plane_counts(npix, edges).astype(np.float64)
    lg, theta, n = np.log2(npix), np.radians(ANGLE), float(npix)
    i, j, k = tr[:, 0], tr[:, 1], tr[:, 2]
    nz = exact > 0
    assert nz.any()
    for s, kappa in enumerate(kappa_maps(out, zs, npix)):
        got = table[:, 7 + s]
        assert np.array_equal(np.isnan(got), ~nz)
        ref = bispectrum_np.bispectrum(kappa, ANGLE, edges, tr)
        eps = 1e-12 * lg * np.linalg.norm(kappa.astype(np.float64))
        r = np.sqrt(np.mean(ref["F"] ** 2, axis=(1, 2)))
        e = eps * N / n ** 2 + 1e-12 * lg * r
        with np.errstate(invalid="ignore", divide="ignore"):
            bound = theta ** 4 / n ** 2 / ref["triangles"] * n ** 2 * (e[i] * r[j] * r[k] + r[i] * e[j] * r[k] +
                                                                       r[i] * r[j] * e[k]) + 1e-13 * np.abs(ref["b"])
        err = np.abs(got - ref["b"])
        assert np.all(err[nz] <= bound[nz]), (s, float(np.max(err[nz] / bound[nz])))
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [32, 30])
def test_bispectrum_file_matches_the_restatement_of_the_kappa_files(tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    edges = ",".join(map(str, EDGES))
    r = run([ini, "--ngp", "--kappa", "0.05,0.1,0.2", "--bispectrum", "all", "--bispectrum-edges", edges])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, "all", EDGES) == 3
    with_bl = files(out, ".kappa_z")
    os.remove(bl_file(out, npix))
    clear(out)
    r = run([ini, "--ngp", "--kappa", "0.05,0.1,0.2", "--bispectrum", "equilateral", "--bispectrum-edges", edges])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, "equilateral", EDGES) == 3
    assert files(out, ".kappa_z") == with_bl
    # without --bispectrum the kappa files are byte-identical and no bispectrum file appears
    os.remove(bl_file(out, npix))
    clear(out)
    r = run([ini, "--ngp", "--kappa", "0.05,0.1,0.2"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, ".kappa_z") == with_bl and not files(out, ".bl_")


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args", [
    (32, ["--bispectrum", "all", "--bispectrum-edges", "0,2,4"]),
    (32, ["--kappa", "all", "--bispectrum", "all"]),
    (32, ["--kappa", "all", "--bispectrum-edges", "0,2,4"]),
    (32, ["--kappa", "all", "--bispectrum", "all", "--bispectrum-edges", ",".join(str(0.25 * i) for i in range(34))]),
    (37, ["--kappa", "all", "--bispectrum", "all", "--bispectrum-edges", "0,2,4"]),
    (32, ["--kappa", "all", "--bispectrum", "isosceles", "--bispectrum-edges", "0,2,4"]),
    (32, ["--kappa", "all", "--bispectrum", "all", "--bispectrum-edges", "3,1"]),
    (32, ["--kappa", "all", "--bispectrum", "all", "--bispectrum-edges", "0,x"]),
])
def test_bispectrum_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "bispectrum" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".bl_" in f]
