"""SLICER_amd --kappa ... --minkowski lo,hi,bins: the table written by the driver against the numpy
restatement (tests/minkowski_np.py) applied to the kappa files of the same run and to their block-mean pyramid
(tests/moments_np.py).  Every count is compared exactly."""
import os

import numpy as np
import pytest

import minkowski_np as MK
import moments_np as M
import peaks_np as P
from test_driver import make_cone, run
from test_driver_peaks import ANGLE, choose_range, kappa_maps, spec
from test_driver_shear import clear, files, read_fits

BINS = 16
KINDS = (".kappa_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".phi_z", ".plane_", ".cl_", ".moments_", ".peaks_")
COLUMNS = ["z", "level", "npix", "j", "threshold", "n_faces", "n_edges", "n_vertices", "n_boundary", "n_border", "euler",
           "n_nan"]


def table_file(out, npix, token=".minkowski_"):
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
    """The T rows of one (source, level) against the restatement of the map x."""
    T, n = t.size, x.shape[0]
    assert rows.shape == (T, len(COLUMNS))
    assert np.all(rows[:, 0] == z) and np.all(rows[:, 1] == level) and np.all(rows[:, 2] == n)
    assert np.array_equal(rows[:, 3], np.arange(T)) and rows[:, 4].tobytes() == t.tobytes()
    ref = MK.counts(x, t)
    for col, name in ((5, "faces"), (6, "edges"), (7, "vertices"), (8, "boundary"), (9, "border"), (10, "euler")):
        assert np.all(rows[:, col] == np.round(rows[:, col]))
        assert np.array_equal(rows[:, col].astype(np.int64), ref[name]), (z, level, name)
    assert np.all(rows[:, 11] == ref["nan"])
    assert np.array_equal(rows[:, 10], rows[:, 7] - rows[:, 6] + rows[:, 5])  # euler = V - E + F in every row
    return ref


def check_against_kappa_files(out, npix, levels, lo, hi):
    t, table = read_table(table_file(out, npix), npix, levels, lo, hi)
    T = t.size
    assert table.shape[0] % ((levels + 1) * T) == 0
    S = table.shape[0] // ((levels + 1) * T)
    maps = kappa_maps(out, npix)
    assert len(maps) == S
    partly = np.zeros(T, bool)
    for s in range(S):
        z = table[s * (levels + 1) * T, 0]
        pyr = M.pyramid(maps[f"{z:.4f}"], levels, "mean")
        for l, x in enumerate(pyr):
            assert x.shape[0] == npix >> l
            ref = check_block(table[(s * (levels + 1) + l) * T:(s * (levels + 1) + l + 1) * T], x, t, z, l)
            if l == 0:
                partly |= (ref["faces"] > 0) & (ref["faces"] < npix * npix)
    # the thresholds were chosen from these maps: a comparison of empty or of full sets alone cannot pass
    assert int(partly.sum()) >= 4
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix,levels", [(32, 5), (30, 4), (37, 0)])
def test_minkowski_file_matches_the_restatement_of_the_kappa_files(tmp_path, npix, levels):
    ini, _, out = make_cone(tmp_path, npix=npix)
    extra = ["--shear", "--power", "auto", "--moments", "--moments-levels", str(levels)] if npix != 37 else []
    args = [ini, "--ngp", "--kappa", "all", "--peaks", "-0.01,0.05,8"] + extra  # (37: no --moments, so level 0 only)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    without = {k: files(out, k) for k in KINDS}
    assert len(without[".kappa_z"]) >= 20 and len(without[".moments_"]) == (1 if extra else 0)
    assert len(without[".peaks_"]) == 1 and not files(out, "minkowski")
    lo, hi = choose_range(out, npix)
    clear(out)
    r = run(args + ["--minkowski", spec(lo, hi)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, levels, lo, hi) >= 20
    # plane, kappa, shear, spectrum, moments and histogram files are byte-identical with and without --minkowski
    assert {k: files(out, k) for k in KINDS} == without
    assert list(files(out, "minkowski")) == [os.path.basename(table_file(out, npix))]


@pytest.mark.gpu
def test_the_four_tables_with_smoothing_and_shape_noise(tmp_path):
    npix = 30
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "1", "--smooth", "gauss:4,8",
            "--shape-noise", "0.3,30,7,2", "--peaks", "-0.01,0.05,8"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not files(out, "minkowski")
    lo, hi = choose_range(out, npix)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + ["--minkowski", spec(lo, hi)])
    assert r.returncode == 0, r.stderr[-2000:]
    # every other file is byte-identical with and without --minkowski
    assert {f: b for f, b in files(out, "").items() if "minkowski" not in f} == without
    assert sorted(files(out, "minkowski")) == sorted(os.path.basename(table_file(out, npix, k)) for k in (
        ".minkowski_", ".smooth_minkowski_", ".noisy_minkowski_", ".noisy_smooth_minkowski_"))
    check_against_kappa_files(out, npix, 1, lo, hi)
    zs = sorted(kappa_maps(out, npix))

    def fits_map(token, z):
        return read_fits(os.path.join(out, f"cone_gadget{token}{z}_{npix}_t0.fits"), npix)[1]

    # the tables of the smoothed, the noisy and the smoothed noisy maps: their leading columns, and every block against
    # the restatement of the map file it was measured on and of its block means
    for token, lead, name in ((".smooth_minkowski_", ("scale",), lambda v: f".gauss{v[0]}_kappa_z"),
                              (".noisy_minkowski_", ("real",), lambda v: f".noisy{v[0]}_kappa_z"),
                              (".noisy_smooth_minkowski_", ("real", "scale"), lambda v: f".noisy{v[0]}_gauss{v[1]}_kappa_z")):
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
def test_minkowski_file_is_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path)
    base = [ini, "--accum", "fixed64", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "3"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    lo, hi = choose_range(out, 32)
    args = base + ["--minkowski", spec(lo, hi)]
    clear(out)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, 32, 3, lo, hi) == 2
    one = open(table_file(out, 32), "rb").read()
    # resume: some plane files removed, the others read back; the table is left in place and rewritten
    for f in files(out, ".kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    with open(table_file(out, 32), "w") as f:
        f.write("stale\n")
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert open(table_file(out, 32), "rb").read() == one
    clear(out)
    os.remove(table_file(out, 32))
    r = run(args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(table_file(out, 32), "rb").read() == one


@pytest.mark.gpu
@pytest.mark.parametrize("args", [
    ["--minkowski", "-0.01,0.05,16"],                      # without --kappa
    ["--kappa", "all", "--minkowski", "-0.01,0.05"],       # not three numbers
    ["--kappa", "all", "--minkowski", "-0.01,0.05,16,2"],
    ["--kappa", "all", "--minkowski", "-0.01,x,16"],
    ["--kappa", "all", "--minkowski", "-0.01,,16"],
    ["--kappa", "all", "--minkowski", "-0.01,0.05,0"],     # bins outside 1 ... 1024
    ["--kappa", "all", "--minkowski", "-0.01,0.05,1025"],
    ["--kappa", "all", "--minkowski", "-0.01,0.05,1.5"],
    ["--kappa", "all", "--minkowski", "0.05,-0.01,16"],    # not ascending
    ["--kappa", "all", "--minkowski", "0.05,0.05,16"],
    ["--kappa", "all", "--minkowski", "0,inf,16"],
    ["--kappa", "all", "--minkowski"],
])
def test_minkowski_is_refused_before_any_plane(tmp_path, args):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--minkowski" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or "minkowski" in f or ".moments_" in f]
