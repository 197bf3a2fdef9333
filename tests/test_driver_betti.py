"""SLICER_amd --kappa ... --betti lo,hi,bins: the tables written by the driver against the labelling
of tests/betti_np.py applied to the kappa files of the same run and to their block-mean pyramid (tests/moments_np.py),
and row by row against the --minkowski table of the same thresholds.  Every count is compared exactly."""
import os

import numpy as np
import pytest

import betti_np as BT
import moments_np as M
import peaks_np as P
from test_driver import make_cone, run
from test_driver_minkowski import read_table as read_minkowski_table
from test_driver_minkowski import table_file as minkowski_file
from test_driver_peaks import ANGLE, choose_range, kappa_maps, spec
from test_driver_shear import files, read_fits

BINS = 16
COLUMNS = ["z", "level", "npix", "j", "threshold", "n_components", "n_holes", "n_faces", "n_nan"]


def table_file(out, npix, token=".betti_"):
    return os.path.join(out, f"cone_gadget{token}{npix}_t0.txt")


def read_table(path, npix, levels, lo, hi, lead=(), bins=BINS):
    """(thresholds, rows) of a table after its '#' lines have been checked; `lead`: the names of the leading columns."""
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    assert head[0] == ["npix", str(npix)] and head[1][0] == "angle_deg" and float(head[1][1]) == ANGLE
    assert head[2] == ["levels", str(levels)]
    t = P.uniform_edges(lo, hi, bins)
    assert head[3][0] == "thresholds" and np.array([float(v) for v in head[3][1:]]).tobytes() == t.tobytes()
    assert head[-1] == list(lead) + COLUMNS
    table = np.loadtxt(path, ndmin=2)
    assert table.shape[1] == len(lead) + len(COLUMNS)
    return t, table


def check_block(rows, x, t, z, level):
    """The T rows of one (source, level) against the labelling of the map x."""
    T, n = t.size, x.shape[0]
    assert rows.shape == (T, len(COLUMNS))
    assert np.all(rows[:, 0] == z) and np.all(rows[:, 1] == level) and np.all(rows[:, 2] == n)
    assert np.array_equal(rows[:, 3], np.arange(T)) and rows[:, 4].tobytes() == t.tobytes()
    ref = BT.counts(x, t)
    for col, name in ((5, "components"), (6, "holes"), (7, "faces")):
        assert np.all(rows[:, col] == np.round(rows[:, col]))
        assert np.array_equal(rows[:, col].astype(np.int64), ref[name]), (z, level, name)
    assert np.all(rows[:, 8] == ref["nan"])
    return ref


def check_against_kappa_files(out, npix, levels, lo, hi):
    t, table = read_table(table_file(out, npix), npix, levels, lo, hi)
    T = t.size
    assert table.shape[0] % ((levels + 1) * T) == 0
    S = table.shape[0] // ((levels + 1) * T)
    maps = kappa_maps(out, npix)
    assert len(maps) == S
    several, holed = np.zeros(T, bool), np.zeros(T, bool)
    for s in range(S):
        z = table[s * (levels + 1) * T, 0]
        pyr = M.pyramid(maps[f"{z:.4f}"], levels, "mean")
        for l, x in enumerate(pyr):
            assert x.shape[0] == npix >> l
            ref = check_block(table[(s * (levels + 1) + l) * T:(s * (levels + 1) + l + 1) * T], x, t, z, l)
            if l == 0:
                several |= ref["components"] > 1
                holed |= ref["holes"] > 0
    # the thresholds were chosen from these maps: a comparison of empty or of full sets alone cannot pass
    assert int(several.sum()) >= 4 and holed.any()
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix,levels", [(32, 5), (37, 0)])
def test_betti_file_matches_the_labelling_and_the_minkowski_table(tmp_path, npix, levels):
    ini, _, out = make_cone(tmp_path, npix=npix)
    extra = ["--shear", "--power", "auto", "--moments", "--moments-levels", str(levels)] if npix != 37 else []
    base = [ini, "--ngp", "--kappa", "all", "--peaks", "-0.01,0.05,8"] + extra  # (37: no --moments, so level 0 only)
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    lo, hi = choose_range(out, npix)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    args = base + ["--minkowski", spec(lo, hi)]
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not files(out, "betti")
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(args + ["--betti", spec(lo, hi)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, levels, lo, hi) >= 20
    # every other file is byte-identical with and without --betti
    assert {f: b for f, b in files(out, "").items() if "betti" not in f} == without
    assert list(files(out, "betti")) == [os.path.basename(table_file(out, npix))]
    # row by row: components - holes is the Euler count of the pixel complex, and the faces are the same
    _, b = read_table(table_file(out, npix), npix, levels, lo, hi)
    _, m = read_minkowski_table(minkowski_file(out, npix), npix, levels, lo, hi)
    assert b.shape[0] == m.shape[0] and np.array_equal(b[:, :5], m[:, :5])
    assert np.array_equal(b[:, 5] - b[:, 6], m[:, 10]) and np.array_equal(b[:, 7], m[:, 5]) and np.array_equal(b[:, 8], m[:, 11])


@pytest.mark.gpu
def test_the_four_tables_with_smoothing_and_shape_noise(tmp_path):
    npix = 30
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "1", "--smooth", "gauss:4,8",
            "--shape-noise", "0.3,30,7,2", "--peaks", "-0.01,0.05,8", "--starlet", "2:-0.01,0.05,4"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not files(out, "betti")
    lo, hi = choose_range(out, npix)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + ["--betti", spec(lo, hi)])
    assert r.returncode == 0, r.stderr[-2000:]
    # every other file is byte-identical with and without --betti
    assert {f: b for f, b in files(out, "").items() if "betti" not in f} == without
    assert sorted(files(out, "betti")) == sorted(os.path.basename(table_file(out, npix, k)) for k in (
        ".betti_", ".smooth_betti_", ".noisy_betti_", ".noisy_smooth_betti_"))
    # the Betti tables are announced after every other file of the run
    said = [ln for ln in r.stdout.splitlines() if ln.startswith("Saving the ")]
    first = min(i for i, ln in enumerate(said) if "betti_" in ln)
    assert all("betti_" in ln for ln in said[first:]) and len(said) - first == 4
    t, table = read_table(table_file(out, npix), npix, 1, lo, hi)
    zs = sorted(kappa_maps(out, npix))
    assert table.shape[0] == len(zs) * 2 * t.size

    def fits_map(token, z):
        return read_fits(os.path.join(out, f"cone_gadget{token}{z}_{npix}_t0.fits"), npix)[1]

    # the four tables: their leading columns, and every block against the labelling of the map file it was measured on
    # and of its block means
    for token, lead, name in ((".betti_", (), lambda v: ".kappa_z"),
                              (".smooth_betti_", ("scale",), lambda v: f".gauss{v[0]}_kappa_z"),
                              (".noisy_betti_", ("real",), lambda v: f".noisy{v[0]}_kappa_z"),
                              (".noisy_smooth_betti_", ("real", "scale"), lambda v: f".noisy{v[0]}_gauss{v[1]}_kappa_z")):
        t, table = read_table(table_file(out, npix, token), npix, 1, lo, hi, lead)
        T, nl = t.size, len(lead)
        blocks = table.reshape(-1, T, table.shape[1])
        assert blocks.shape[0] == len(zs) * 2 * 2 ** nl  # sources x levels x (scales, realisations: two of each)
        seen = set()
        for b in blocks:
            v = tuple(int(c) for c in b[0, :nl])
            assert np.all(b[:, :nl] == b[0, :nl])
            z, level = b[0, nl], int(b[0, nl + 1])
            seen.add((v, f"{z:.4f}", level))
            x = M.pyramid(fits_map(name(v), f"{z:.4f}"), 1, "mean")[level]
            check_block(b[:, nl:], x, t, z, level)
        assert len(seen) == blocks.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("args,message", [
    (["--betti", "-0.01,0.05,16"], "--betti needs --kappa (the Betti numbers are those of the kappa maps)"),
    (["--kappa", "all", "--betti", "-0.01,0.05"], "--betti"),          # not three numbers
    (["--kappa", "all", "--betti", "-0.01,0.05,1025"], "--betti"),     # bins outside 1 ... 1024
    (["--kappa", "all", "--betti", "0.05,-0.01,16"], "--betti"),       # not ascending
    (["--kappa", "all", "--betti"], "--betti"),
])
def test_betti_is_refused_before_any_plane(tmp_path, args, message):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert message in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or "betti" in f or ".moments_" in f]
