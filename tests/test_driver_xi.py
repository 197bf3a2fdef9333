"""SLICER_amd --kappa ... --xi: the correlation-function tables written by the driver against
slicer_amd.Xi applied to the kappa and gamma files of the same run: the same device code on the same f32 maps, so the
tables agree to the printed digits."""
import os

import numpy as np
import pytest

import slicer_amd
from slicer_amd import fits
from test_driver import make_cone, run
from test_driver_power import kappa_maps
from test_driver_shear import read_fits

ANGLE = 2.0  # make_cone's field of view
NPIX = 32
ARCMIN = 60.0 * ANGLE / NPIX  # of one pixel
EDGES = [0.0, 3.75, 7.5, 10.0, 20.0, 41.25, 60.0]  # arcminutes: 0, 1, 2, 2.67, 5.33, 11, 16 pixels
E = ",".join(map(str, EDGES))
ZS = [0.05, 0.1, 0.2]


def table(out, token):
    path = os.path.join(out, f"cone_gadget.{token}_{NPIX}_t0.txt")
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    return {h[0]: h[1:] for h in head[:-1]}, head[-1], np.loadtxt(path, ndmin=2)


def mask_file(tmp_path):
    w = (np.random.default_rng(3).random((NPIX, NPIX)) < 0.7).astype(np.float32)
    w[:4, 20:] = 0.0
    path = str(tmp_path / "xi_mask.fits")
    fits.write_image(path, w, [])
    return path, w


def gamma_maps(out, z):
    maps = []
    for k in (1, 2):
        name = [f for f in os.listdir(out) if f.startswith(f"cone_gadget.gamma{k}_z{z:.4f}_")]
        assert len(name) == 1
        maps.append(read_fits(os.path.join(out, name[0]), NPIX)[1])
    return maps


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_xi_tables_equal_the_api_on_the_written_maps(tmp_path, masked):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    path, w = mask_file(tmp_path)
    args = [ini, "--ngp", "--kappa", ",".join(map(str, ZS)), "--shear", "--xi", "cross", "--xi-edges", E]
    r = run(args + (["--xi-mask", path] if masked else []))
    assert r.returncode == 0, r.stderr[-2000:]
    edges_pix = np.asarray(EDGES, np.float64) * NPIX / (60.0 * ANGLE)
    bins = slicer_amd.xi_bins(NPIX, edges_pix)
    S, B = len(ZS), len(EDGES) - 1
    pairs = [(s, t) for s in range(S) for t in range(s, S)]
    meta, cols, tab = table(out, "xi")
    assert meta["npix"] == [str(NPIX)] and float(meta["angle_deg"][0]) == ANGLE
    assert [float(z) for z in meta["zs"]] == ZS
    assert meta["mask"] == ([path] if masked else ["none"]) and meta["padded"] == [str(bins["padded"])]
    assert cols == ["r_lo", "r_hi", "r_mean"] + [f"xi_{s}_{t}" for s, t in pairs] + ["weight", "n_pairs"]
    assert tab.shape == (B, 3 + len(pairs) + 2)
    metap, colsp, tabp = table(out, "xipm")
    assert metap == meta
    assert colsp == ["r_lo", "r_hi", "r_mean"] + [c for s in range(S) for c in (f"xip_{s}", f"xim_{s}")] + ["weight", "n_pairs"]
    kappas = kappa_maps(out, ZS, NPIX)
    with slicer_amd.Slicer(0) as sl:
        dw = sl.to_device(w) if masked else None
        with slicer_amd.Xi(sl, NPIX, 0, S, edges_pix, cross=True) as x:
            x.set_weights(dw)
            d = [sl.to_device(np.ascontiguousarray(k, np.float32)) for k in kappas]
            x.run(d)
            ref = x.read()
        for t_ in (tab, tabp):
            assert same(t_[:, 0], EDGES[:-1]) and same(t_[:, 1], EDGES[1:])
            assert same(t_[:, 2], ref["r"] * ARCMIN)
            assert same(t_[:, -2], ref["weights"]) and same(t_[:, -1], bins["counts"])
        for q, (s, t) in enumerate(pairs):
            assert same(tab[:, 3 + q], ref["xi"][s, t]), (s, t)
        assert not np.isnan(tab[1:, 3:-2]).any() and np.isnan(tab[0, 3]) == (bins["lags"][0] == 0)
        with slicer_amd.Xi(sl, NPIX, 2, 1, edges_pix) as x:
            x.set_weights(dw)
            for s, z in enumerate(ZS):
                x.run([sl.to_device(np.ascontiguousarray(g, np.float32)) for g in gamma_maps(out, z)])
                ref = x.read()
                assert same(tabp[:, 3 + 2 * s], ref["xip"][0]), s
                assert same(tabp[:, 4 + 2 * s], ref["xim"][0]), s
    # auto: the diagonal of cross, and no .xipm_ table without --shear
    for f in os.listdir(out):
        if f.endswith(".fits") or ".xi" in f:
            os.remove(os.path.join(out, f))
    r = run([ini, "--ngp", "--kappa", ",".join(map(str, ZS)), "--xi", "auto", "--xi-edges", E] +
            (["--xi-mask", path] if masked else []))
    assert r.returncode == 0, r.stderr[-2000:]
    _, cols_a, tab_a = table(out, "xi")
    assert cols_a == ["r_lo", "r_hi", "r_mean"] + [f"xi_{s}_{s}" for s in range(S)] + ["weight", "n_pairs"]
    for s in range(S):
        assert same(tab_a[:, 3 + s], tab[:, 3 + pairs.index((s, s))])
    assert not [f for f in os.listdir(out) if ".xipm_" in f]


@pytest.mark.gpu
@pytest.mark.parametrize("args,message", [
    (["--xi", "auto", "--xi-edges", E], "--xi needs --kappa"),
    (["--kappa", "all", "--xi", "both", "--xi-edges", E], "bad --xi (auto or cross)"),
    (["--kappa", "all", "--xi", "auto"], "--xi needs --xi-edges"),
    (["--kappa", "all", "--xi-edges", E], "--xi-edges needs --xi"),
    (["--kappa", "all", "--xi-mask", "MASK16"], "--xi-mask needs --xi"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", "0,x"], "bad --xi-edges (a comma-separated list of radii in arcminutes)"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", ",".join(str(0.1 * i) for i in range(514))],
     "bad --xi-edges (514 edges, at most 513)"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", "10,5"], "--xi-edges: slicer_xi_bins: edges must be strictly ascending"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", "5"], "--xi-edges: slicer_xi_bins: fewer than 2 edges"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", "-1,5"], "--xi-edges: slicer_xi_bins: edges must be finite and non-negative"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", "0,170"],
     "--xi-edges: slicer_xi_bins: the last edge is beyond sqrt(2) (npix - 1)"),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", E, "--xi-mask", "missing.fits"], "--xi-mask: "),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", E, "--xi-mask", "MASK16"], "--xi-mask: "),
    (["--kappa", "all", "--xi", "auto", "--xi-edges", E, "--xi-mask", "MASKNEG"], "slicer_amd: --xi"),
])
def test_xi_is_refused_before_any_plane(tmp_path, args, message):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    small = str(tmp_path / "mask16.fits")
    fits.write_image(small, np.ones((16, 16), np.float32), [])
    neg = str(tmp_path / "maskneg.fits")
    w = np.ones((NPIX, NPIX), np.float32)
    w[3, 5] = -0.5
    fits.write_image(neg, w, [])
    args = [{"MASK16": small, "MASKNEG": neg}.get(a, a) for a in args]
    r = run([ini] + args)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr[-1000:]
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".xi" in f]


@pytest.mark.gpu
def test_xi_is_refused_for_a_physical_run(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=-150)  # a physical pixel size: no angle
    r = run([ini, "--kappa", "all", "--xi", "auto", "--xi-edges", E])
    assert r.returncode != 0
    assert "--xi-edges: the edges are angles, and the maps of a physical run have none" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".xi" in f]
