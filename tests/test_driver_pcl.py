"""SLICER_amd --kappa ... --pcl: the pseudo-C_l and coupling-matrix files written by the driver
against the numpy restatement (tests/pcl_np.py) applied to the kappa files of the same run."""
import os

import numpy as np
import pytest

import pcl_np
import power_np
import slicer_amd
from slicer_amd import fits
from test_driver import make_cone, run
from test_driver_power import kappa_maps
from test_driver_shear import clear, files
from test_gpu_pcl import C_M, holes

ANGLE = 2.0  # make_cone's field of view
NPIX = 32
EDGES = [0, 1, 2, 3, 4.5, 6, 8, 11, 16, 23]
TAPER_ARCMIN = 15.0  # 4 pixels
OTHERS = (".kappa_z", ".gamma1_z", ".phi_z", ".plane_", ".cl_")


def table_file(out, token):
    return os.path.join(out, f"cone_gadget.{token}_{NPIX}_t0.txt")


def pcl_args(mode, mask_path, kind="cross"):
    args = ["--pcl", kind, "--pcl-edges", ",".join(map(str, EDGES))]
    if mode in ("taper", "both"):
        args += ["--pcl-taper", str(TAPER_ARCMIN)]
    if mode in ("mask", "both"):
        args += ["--pcl-mask", mask_path]
    return args


def write_mask(tmp_path, bitpix=-32):
    path = str(tmp_path / f"mask{bitpix}.fits")
    fits.write_image(path, holes(NPIX), [], bitpix=bitpix)
    return path


def parse(out):
    path = table_file(out, "pcl")
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    meta = {h[0]: h[1:] for h in head[:-1]}
    return meta, head[-1], np.loadtxt(path, ndmin=2), np.loadtxt(table_file(out, "pclm"), ndmin=2)


def check_against_kappa_files(out, mode, mask_path, cross):
    meta, cols, table, M = parse(out)
    assert meta["npix"] == [str(NPIX)] and float(meta["angle_deg"][0]) == ANGLE
    zs = [float(z) for z in meta["zs"]]
    S = len(zs)
    pairs = power_np.pairs(S, cross)
    assert cols == ["ell_lo", "ell_hi", "ell_mean", "n_modes"] + [c for s, t in pairs for c in (f"C_{s}_{t}", f"Ct_{s}_{t}")]
    edges = np.asarray(EDGES, np.float64)
    B = edges.size - 1
    assert table.shape == (B, 4 + 2 * len(pairs)) and M.shape == (B, B)
    ell_f = slicer_amd.ell_fundamental(ANGLE)
    assert np.array_equal(table[:, 0], edges[:-1] * ell_f) and np.array_equal(table[:, 1], edges[1:] * ell_f)
    bins = slicer_amd.power_bins(NPIX, edges)
    assert np.array_equal(table[:, 3].astype(np.int64), bins["counts"])
    assert np.array_equal(table[:, 2], bins["mean_radius"] * ell_f, equal_nan=True)
    # the mask and its header lines
    width = TAPER_ARCMIN * NPIX / (60.0 * ANGLE) if mode != "mask" else 0.0
    assert float(meta["taper_pix"][0]) == width and float(meta["taper_arcmin"][0]) == (TAPER_ARCMIN if width else 0.0)
    assert meta["mask"] == ([mask_path] if mode != "taper" else ["none"])
    w = pcl_np.mask(NPIX, width, holes(NPIX) if mode != "taper" else None)
    w64 = w.astype(np.float64)
    N = float(NPIX * NPIX)
    assert abs(float(meta["mean_w"][0]) - w64.mean()) <= 2 * N * 2.0 ** -53 * w64.mean()
    assert abs(float(meta["mean_w2"][0]) - (w64 ** 2).mean()) <= 2 * N * 2.0 ** -53 * (w64 ** 2).mean()
    # M: the bound of tests/test_gpu_pcl.py
    assert np.abs(M - pcl_np.coupling_fft(w, edges)).max() <= C_M * 1e-12 * np.log2(NPIX) * (w64 ** 2).mean()
    # the coupled bandpowers: the bound of tests/test_driver_power.py for the multiplied maps
    maps = [w * m for m in kappa_maps(out, zs, NPIX)]
    exact = [np.fft.rfft2(m.astype(np.float64)) for m in maps]
    ref = power_np.power_of_spectra(exact, ANGLE, edges, cross=True)
    nz = ref["counts"] > 0
    eps = [1e-12 * np.log2(NPIX) * np.linalg.norm(m.astype(np.float64)) for m in maps]
    counts, mags = power_np.binned_sums(NPIX, edges, [np.abs(x) for x in exact])
    norm = np.radians(ANGLE) ** 2 / float(NPIX) ** 4
    Ma = M[np.ix_(nz, nz)]
    cond = np.linalg.cond(Ma)
    for q, (s, t) in enumerate(pairs):
        cl, coupled = table[:, 4 + 2 * q], table[:, 5 + 2 * q]
        assert np.array_equal(np.isnan(cl), ~nz) and np.array_equal(np.isnan(coupled), ~nz)
        ms, mt = mags[s][nz] / counts[nz], mags[t][nz] / counts[nz]
        bnd = norm * (eps[s] * mt + eps[t] * ms + eps[s] * eps[t]) + 1e-13 * np.abs(ref["cl"][s, t][nz])
        assert np.all(np.abs(coupled[nz] - ref["cl"][s, t][nz]) <= bnd), (s, t)
        # the decoupling: the solve of the file's own M and coupled bandpowers
        solved = np.linalg.solve(Ma, coupled[nz])
        assert np.all(np.abs(cl[nz] - solved) <= 1e-13 * cond * np.abs(coupled[nz]).max()), (s, t)
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["taper", "mask", "both"])
def test_pcl_files_match_the_restatement_of_the_kappa_files(tmp_path, mode):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    mask_path = write_mask(tmp_path, -64 if mode == "both" else -32)
    base = [ini, "--ngp", "--kappa", "0.05,0.1,0.2", "--shear", "--power", "auto"]
    r = run(base + pcl_args(mode, mask_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, mode, mask_path, cross=True) == 3
    if mode != "both":
        return
    # auto, and every other file byte-identical with and without --pcl
    with_pcl = {k: files(out, k) for k in OTHERS}
    assert all(with_pcl.values())
    os.remove(table_file(out, "pcl"))
    os.remove(table_file(out, "pclm"))
    os.remove(table_file(out, "cl"))
    clear(out)
    r = run(base + pcl_args(mode, mask_path, "auto"))
    assert r.returncode == 0, r.stderr[-2000:]
    check_against_kappa_files(out, mode, mask_path, cross=False)
    assert {k: files(out, k) for k in OTHERS} == with_pcl
    os.remove(table_file(out, "pcl"))
    os.remove(table_file(out, "pclm"))
    os.remove(table_file(out, "cl"))
    clear(out)
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: files(out, k) for k in OTHERS} == with_pcl
    assert not files(out, ".pcl")


@pytest.mark.gpu
def test_pcl_files_are_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    mask_path = write_mask(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.2"] + pcl_args("both", mask_path)
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = files(out, ".pcl")
    assert len(one) == 2
    for f in files(out, ".kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    for f in one:
        with open(os.path.join(out, f), "w") as stale:
            stale.write("stale\n")
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert files(out, ".pcl") == one
    clear(out)
    for f in one:
        os.remove(os.path.join(out, f))
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, ".pcl") == one


E = ",".join(map(str, EDGES))


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args", [
    (32, ["--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "15"]),                      # no --kappa
    (37, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "15"]),    # not an FFT size
    (32, ["--kappa", "all", "--pcl", "both", "--pcl-edges", E, "--pcl-taper", "15"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-taper", "15"]),                      # no edges
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E]),                         # neither taper nor mask
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", "3,1", "--pcl-taper", "15"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", "0,x", "--pcl-taper", "15"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", ",".join(str(0.01 * i) for i in range(514)), "--pcl-taper", "15"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "0"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "-3"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "nan"]),
    (32, ["--kappa", "all", "--pcl-edges", E]),
    (32, ["--kappa", "all", "--pcl-taper", "15"]),
    (32, ["--kappa", "all", "--pcl-mask", "MASK16"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-mask", "missing.fits"]),
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-mask", "MASK16"]),  # another shape
    (32, ["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-mask", "MASKINT"]),  # BITPIX 32
    (32, ["--kappa", ",".join(f"{0.01 + 0.001 * i:.3f}" for i in range(129)), "--pcl", "cross", "--pcl-edges", E,
          "--pcl-taper", "15"]),
])
def test_pcl_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    small = str(tmp_path / "mask16.fits")
    fits.write_image(small, np.ones((16, 16), np.float32), [])
    ints = str(tmp_path / "maskint.fits")
    with open(ints, "wb") as f:
        f.write(open(write_mask(tmp_path), "rb").read().replace(b"BITPIX  =                  -32",
                                                                 b"BITPIX  =                   32"))
    args = [{"MASK16": small, "MASKINT": ints}.get(a, a) for a in args]
    r = run([ini] + args)
    assert r.returncode != 0
    assert "pcl" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".pcl" in f]
