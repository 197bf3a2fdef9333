"""SLICER_amd --kappa ... --peaks lo,hi,bins: the histogram file written by the driver against the
numpy restatement (tests/peaks_np.py) applied to the kappa files of the same run and to their block-mean pyramid
(tests/moments_np.py).  Every count is compared exactly."""
import os

import numpy as np
import pytest

import moments_np as M
import peaks_np as P
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

ANGLE = 2.0  # make_cone's field of view
BINS = 16
KINDS = (".kappa_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".phi_z", ".plane_", ".cl_", ".moments_")


def peaks_file(out, npix):
    return os.path.join(out, f"cone_gadget.peaks_{npix}_t0.txt")


def kappa_maps(out, npix):
    """{"%.4f" % z: the kappa map} of the run's kappa files."""
    maps = {}
    for f in sorted(os.listdir(out)):
        if f.startswith("cone_gadget.kappa_z"):
            maps[f[len("cone_gadget.kappa_z"):].split("_")[0]] = read_fits(os.path.join(out, f), npix)[1]
    return maps


def choose_range(out, npix):
    """lo, hi from the run's own kappa files: the 3rd and 97th percentile of all level-0 pixels."""
    pixels = np.concatenate([m.ravel() for m in kappa_maps(out, npix).values()]).astype(np.float64)
    lo, hi = (float(v) for v in np.percentile(pixels, [3.0, 97.0]))
    assert lo < hi
    return lo, hi


def spec(lo, hi, bins=BINS):
    return f"{lo!r},{hi!r},{bins}"  # repr round-trips a double


def check_against_kappa_files(out, npix, levels, lo, hi, bins=BINS):
    path = peaks_file(out, npix)
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    assert head[0] == ["npix", str(npix)] and head[1][0] == "angle_deg" and float(head[1][1]) == ANGLE
    assert head[2] == ["levels", str(levels)]
    edges = P.uniform_edges(lo, hi, bins)
    assert head[3][0] == "edges" and np.array([float(v) for v in head[3][1:]]).tobytes() == edges.tobytes()
    assert head[4] == ["z", "level", "npix", "bin", "lo", "hi", "n_pixels", "n_peaks", "n_minima"] and len(head) == 5
    table = np.loadtxt(path, ndmin=2)
    rows_per = bins + 3
    assert table.shape[1] == 9 and table.shape[0] % ((levels + 1) * rows_per) == 0
    S = table.shape[0] // ((levels + 1) * rows_per)
    maps = kappa_maps(out, npix)
    assert len(maps) == S
    inside = nonempty = total0 = 0
    for s in range(S):
        z = table[s * (levels + 1) * rows_per, 0]
        pyr = M.pyramid(maps[f"{z:.4f}"], levels, "mean")
        for l, x in enumerate(pyr):
            n = x.shape[0]
            rows = table[(s * (levels + 1) + l) * rows_per:(s * (levels + 1) + l + 1) * rows_per]
            assert np.all(rows[:, 0] == z) and np.all(rows[:, 1] == l) and np.all(rows[:, 2] == n) and n == npix >> l
            assert np.array_equal(rows[:, 3], np.arange(-1, bins + 2))
            assert rows[0, 4] == -np.inf and rows[-2, 5] == np.inf and np.isnan(rows[-1, 4]) and np.isnan(rows[-1, 5])
            assert rows[1:-1, 4].tobytes() == edges.tobytes() and rows[:-2, 5].tobytes() == edges.tobytes()
            ref = P.counts(x, edges)
            for col, name, k in ((6, "pdf", 0), (7, "peaks", 1), (8, "minima", 2)):
                want = [ref["below"][k]] + list(ref[name]) + [ref["above"][k]] + [ref["nan"] if k == 0 else 0]
                assert np.array_equal(rows[:, col].astype(np.int64), np.array(want, np.int64)), (s, l, name)
                assert np.all(rows[:, col] == np.round(rows[:, col]))
            assert rows[:, 6].sum() == n * n  # every pixel of the level is in one row
            if l == 0:
                inside += ref["pdf"].sum()
                total0 += n * n
                nonempty = np.maximum(nonempty, ref["pdf"] > 0)
    # the edges were chosen from these maps: an all-`below` file cannot pass
    assert inside >= 0.9 * total0, (inside, total0)
    assert int(np.sum(nonempty)) >= 4
    return S


@pytest.mark.gpu
@pytest.mark.parametrize("npix,levels", [(32, 5), (30, 4), (37, 0)])
def test_peaks_file_matches_the_restatement_of_the_kappa_files(tmp_path, npix, levels):
    ini, _, out = make_cone(tmp_path, npix=npix)
    extra = ["--shear", "--power", "auto", "--moments", "--moments-levels", str(levels)] if npix != 37 else []
    args = [ini, "--ngp", "--kappa", "all"] + extra  # (37: no --moments, so level 0 only)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    without = {k: files(out, k) for k in KINDS}
    assert len(without[".kappa_z"]) >= 20 and len(without[".moments_"]) == (1 if extra else 0)
    assert not files(out, ".peaks_")
    lo, hi = choose_range(out, npix)
    clear(out)
    r = run(args + ["--peaks", spec(lo, hi)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, npix, levels, lo, hi) >= 20
    # plane, kappa, shear, spectrum and moments files are byte-identical with and without --peaks
    assert {k: files(out, k) for k in KINDS} == without


@pytest.mark.gpu
def test_peaks_file_is_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path)
    base = [ini, "--accum", "fixed64", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "3"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    lo, hi = choose_range(out, 32)
    args = base + ["--peaks", spec(lo, hi)]
    clear(out)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert check_against_kappa_files(out, 32, 3, lo, hi) == 2
    one = open(peaks_file(out, 32), "rb").read()
    # resume: some plane files removed, the others read back; the peaks file is left in place and rewritten
    for f in files(out, ".kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    with open(peaks_file(out, 32), "w") as f:
        f.write("stale\n")
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert open(peaks_file(out, 32), "rb").read() == one
    clear(out)
    os.remove(peaks_file(out, 32))
    r = run(args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(peaks_file(out, 32), "rb").read() == one


@pytest.mark.gpu
@pytest.mark.parametrize("args", [
    ["--peaks", "-0.01,0.05,16"],                      # without --kappa
    ["--kappa", "all", "--peaks", "-0.01,0.05"],       # not three numbers
    ["--kappa", "all", "--peaks", "-0.01,0.05,16,2"],
    ["--kappa", "all", "--peaks", "-0.01,x,16"],
    ["--kappa", "all", "--peaks", "-0.01,,16"],
    ["--kappa", "all", "--peaks", "-0.01,0.05,0"],     # bins outside 1 ... 1024
    ["--kappa", "all", "--peaks", "-0.01,0.05,1025"],
    ["--kappa", "all", "--peaks", "-0.01,0.05,1.5"],
    ["--kappa", "all", "--peaks", "0.05,-0.01,16"],    # not ascending
    ["--kappa", "all", "--peaks", "0.05,0.05,16"],
    ["--kappa", "all", "--peaks", "0,inf,16"],
    ["--kappa", "all", "--peaks"],
])
def test_peaks_are_refused_before_any_plane(tmp_path, args):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--peaks" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or ".peaks_" in f or ".moments_" in f]
