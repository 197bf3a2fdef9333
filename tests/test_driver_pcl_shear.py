"""SLICER_amd --kappa ... --shear --pcl ... --pcl-shear: the E/B pseudo-C_l and coupling-matrix files written by the
driver against the numpy restatement (tests/pcl_shear_np.py) applied to the kappa and gamma files of
the same run, and the refusals, which need no device."""
import os

import numpy as np
import pytest

import pcl_np
import pcl_shear_np
import power_np
from test_driver import make_cone, run
from test_driver_pcl import ANGLE, EDGES, NPIX, TAPER_ARCMIN, pcl_args, table_file
from test_driver_shear import clear, files, read_fits
from test_gpu_pcl import C_M
from test_gpu_pcl_shear import C_M2

E = ",".join(map(str, EDGES))
MATS = ("M0", "M2", "X2", "M4", "X4")


@pytest.mark.parametrize("args,word", [
    (["--kappa", "all", "--shear", "--pcl-shear"], "--pcl-shear needs --pcl"),
    (["--kappa", "all", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "15", "--pcl-shear"], "--pcl-shear needs --shear"),
    (["--kappa", "all", "--shear", "--pcl", "cross", "--pcl-edges", ",".join(str(0.1 * i) for i in range(130)),
      "--pcl-taper", "15", "--pcl-shear"], "at most 129"),
    (["--shear", "--pcl", "auto", "--pcl-edges", E, "--pcl-taper", "15", "--pcl-shear"], "needs --kappa"),
])
def test_pcl_shear_is_refused_before_any_device_work(tmp_path, args, word):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    r = run([ini] + args)
    assert r.returncode == 2
    assert word in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".pcl" in f]


def source_maps(out, zs, token):
    names = os.listdir(out)
    maps = []
    for z in zs:
        name = [f for f in names if f.startswith(f"cone_gadget.{token}_z{z:.4f}_")]
        assert len(name) == 1, (token, z, name)
        maps.append(read_fits(os.path.join(out, name[0]), NPIX)[1])
    return maps


def parse(out):
    path = table_file(out, "pcleb")
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    meta = {h[0]: h[1:] for h in head[:-1]}
    mats, name = {}, None
    for ln in open(table_file(out, "pclebm")):
        if ln.startswith("#"):
            name = ln[1:].split()[0]
        else:
            mats.setdefault(name, []).append([float(x) for x in ln.split()])
    return meta, head[-1], np.loadtxt(path, ndmin=2), {k: np.array(v) for k, v in mats.items() if k in MATS}


def expected_columns(S, cross):
    cols = []
    for s in range(S):
        for t in (range(s, S) if cross else [s]):
            cols += [f"EE_{s}_{t}", f"EB_{s}_{t}"] + ([f"BE_{s}_{t}"] if s < t else []) + [f"BB_{s}_{t}"]
            cols += [f"kE_{s}_{t}", f"kB_{s}_{t}"] + ([f"kE_{t}_{s}", f"kB_{t}_{s}"] if s < t else [])
    return cols


def check_against_the_map_files(out, cross):
    meta, cols, table, mats = parse(out)
    zs = [float(z) for z in meta["zs"]]
    S = len(zs)
    names = expected_columns(S, cross)
    assert cols == ["ell_lo", "ell_hi", "ell_mean", "n_modes"] + [c for k in names for c in ("C_" + k, "Ct_" + k)]
    edges = np.asarray(EDGES, np.float64)
    B = edges.size - 1
    assert table.shape == (B, 4 + 2 * len(names)) and sorted(mats) == sorted(MATS)
    # the '#' lines and the bin columns are those of the .pcl_ table
    pcl_lines = open(table_file(out, "pcl")).read().split("\n")
    eb_lines = open(table_file(out, "pcleb")).read().split("\n")
    k = [i for i, ln in enumerate(pcl_lines) if ln.startswith("#")][-1]
    assert eb_lines[:k] == pcl_lines[:k]
    pcl = np.loadtxt(table_file(out, "pcl"), ndmin=2)
    assert np.array_equal(table[:, :4], pcl[:, :4], equal_nan=True)
    width = TAPER_ARCMIN * NPIX / (60.0 * ANGLE)
    w = pcl_np.mask(NPIX, width, None)
    kappa, g1, g2 = (source_maps(out, zs, t) for t in ("kappa", "gamma1", "gamma2"))
    fields = [(g1[s], g2[s], kappa[s]) for s in range(S)]
    ref = pcl_shear_np.pcl_shear(fields, w, ANGLE, edges, cross=True)
    nz = ref["counts"] > 0
    ix = np.flatnonzero(nz)
    # the matrices: the bounds of tests/test_gpu_pcl.py and tests/test_gpu_pcl_shear.py
    unit = 1e-12 * np.log2(NPIX) * float((w.astype(np.float64) ** 2).mean())
    assert np.array_equal(mats["M0"], np.loadtxt(table_file(out, "pclm"), ndmin=2))
    for name in MATS:
        assert mats[name].shape == (B, B)
        assert np.abs(mats[name] - ref["matrices"][name]).max() <= (C_M if name == "M0" else C_M2) * unit, name
    # the coupled bandpowers: the spectrum bound of row N6 for every masked map, eps = 1e-12 log2(n) ||w map||_2, which
    # the rotation (|c2|, |s2| <= 1) adds up for E and B, propagated as tests/test_driver_power.py does
    norm = np.radians(ANGLE) ** 2 / float(NPIX) ** 4
    eps, mag = {}, {}
    for s in range(S):
        e = [1e-12 * np.log2(NPIX) * np.linalg.norm((w * m).astype(np.float64)) for m in fields[s]]
        eps[s] = {"E": e[0] + e[1], "B": e[0] + e[1], "k": e[2]}
        _, mg = power_np.binned_sums(NPIX, edges, [np.abs(x) for x in ref["spectra"][s]])
        mag[s] = dict(zip("EBk", (m[nz] / ref["counts"][nz] for m in mg)))
    col = {k: (table[:, 4 + 2 * i], table[:, 5 + 2 * i]) for i, k in enumerate(names)}
    for k, (cl, coupled) in col.items():
        (a, b), s, t = k.split("_")[0], int(k.split("_")[1]), int(k.split("_")[2])
        assert np.array_equal(np.isnan(cl), ~nz) and np.array_equal(np.isnan(coupled), ~nz), k
        want = ref["coupled"][a + b][s, t][nz]
        bnd = norm * (eps[s][a] * mag[t][b] + eps[t][b] * mag[s][a] + eps[s][a] * eps[t][b]) + 1e-13 * np.abs(want)
        assert np.all(np.abs(coupled[nz] - want) <= bnd), k
    # the decoupling: the block solves of the file's own matrices and coupled bandpowers
    s4 = pcl_shear_np.system4(mats["M0"], mats["M4"], mats["X4"])
    s2 = pcl_shear_np.system2(mats["M2"], mats["X2"])

    def cond(system, m):
        idx = np.concatenate([j * B + ix for j in range(m)])
        return np.linalg.cond(system[np.ix_(idx, idx)])
    c4, c2 = cond(s4, 4), cond(s2, 2)
    for s in range(S):
        for t in (range(s, S) if cross else [s]):
            four = [f"EE_{s}_{t}", f"EB_{s}_{t}", f"BE_{s}_{t}" if s < t else f"EB_{s}_{t}", f"BB_{s}_{t}"]
            groups = [(s4, c4, four), (s2, c2, [f"kE_{s}_{t}", f"kB_{s}_{t}"])]
            if s < t:
                groups.append((s2, c2, [f"kE_{t}_{s}", f"kB_{t}_{s}"]))
            for system, cnd, members in groups:
                solved = pcl_shear_np.solve_blocks(system, [col[k][1] for k in members], nz)
                scale = max(np.abs(col[k][1][nz]).max() for k in members)
                for k, x in zip(members, solved):
                    assert np.all(np.abs(col[k][0][nz] - x[nz]) <= 1e-13 * cnd * scale), k
    return S


@pytest.mark.gpu
def test_pcleb_files_match_the_restatement_of_the_map_files(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--shear", "--power", "auto"]
    r = run(base + pcl_args("taper", None) + ["--pcl-shear"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_the_map_files(out, cross=True) == 2
    # every other file of the run, byte for byte, with and without --pcl-shear
    with_eb = {f: b for f, b in files(out, "").items() if ".pcleb" not in f}
    assert len(files(out, ".pcleb")) == 2 and any(".pcl_" in f for f in with_eb) and any(".gamma1_z" in f for f in with_eb)
    for f in files(out, ".pcl"):
        os.remove(os.path.join(out, f))
    os.remove(table_file(out, "cl"))
    clear(out)
    r = run(base + pcl_args("taper", None))
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, "") == with_eb
    # auto: the pairs within each source
    for f in files(out, ".pcl"):
        os.remove(os.path.join(out, f))
    os.remove(table_file(out, "cl"))
    clear(out)
    r = run(base + pcl_args("taper", None, "auto") + ["--pcl-shear"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_the_map_files(out, cross=False) == 2
