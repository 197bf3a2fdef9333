"""SLICER_amd --kappa ... --catalogue min_peak[,capacity]: the peak tables written by the driver
against the numpy restatement (tests/catalogue_np.py) applied to the kappa files of the same run -- the plain, the
smoothed, the noisy and the smoothed noisy ones.  Every number is compared exactly."""
import os

import numpy as np
import pytest

import catalogue_np as K
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

pytestmark = pytest.mark.gpu

ANGLE = 2.0  # make_cone's field of view
NPIX = 32
ZS = ("0.05", "0.2")
SCALES = (2.0, 5.625)  # arcminutes
NREAL = 2
DEFAULT_CAPACITY = 1 << 20
BASE = ["--ngp", "--kappa", ",".join(ZS), "--smooth", "gauss:" + ",".join(repr(a) for a in SCALES),
        "--shape-noise", f"0.26,30.0,7,{NREAL}"]
# family: (file token, the columns after z, (prefix of the map's FITS file, the values of those columns) per map of a source)
FAMILIES = {
    "": ((), [("kappa", ())]),
    "smooth_": (("scale",), [(f"gauss{k}_kappa", (k,)) for k in range(len(SCALES))]),
    "noisy_": (("real",), [(f"noisy{r}_kappa", (r,)) for r in range(NREAL)]),
    "noisy_smooth_": (("real", "scale"), [(f"noisy{r}_gauss{k}_kappa", (r, k)) for r in range(NREAL) for k in range(len(SCALES))]),
}


def table_path(out, family):
    return os.path.join(out, f"cone_gadget.{family}catalogue_{NPIX}_t0.txt")


def load_map(out, prefix, z):
    return read_fits(os.path.join(out, f"cone_gadget.{prefix}_z{float(z):.4f}_{NPIX}_t0.fits"), NPIX)[1]


def expected_rows(x, z, lead, min_peak, capacity):
    """(the rows of the map's table, the number of its peaks)."""
    rec = K.catalogue(x, K.PEAKS, min_peak)
    total = len(rec)
    rec = rec[:capacity]
    row, col = rec["row"].astype(np.float64), rec["col"].astype(np.float64)
    off = [(((p + d) + 0.5) / np.float64(NPIX) - 0.5) * np.float64(ANGLE) for p, d in ((row, rec["dy"]), (col, rec["dx"]))]
    cols = [np.full(len(rec), float(z))] + [np.full(len(rec), float(v)) for v in lead]
    cols += [row, col, rec["value"].astype(np.float64), rec["dy"], rec["dx"], off[0], off[1], rec["flags"].astype(np.float64)]
    return np.stack(cols, axis=1) if len(rec) else np.zeros((0, len(cols))), total


def check_family(out, family, min_peak, capacity):
    """The family's table against the restatement of the run's own FITS files -> (peaks of all its maps, rows)."""
    lead_names, maps = FAMILIES[family]
    path = table_path(out, family)
    lines = open(path).read().split("\n")
    head = [ln[1:].split() for ln in lines if ln.startswith("#")]
    fixed = [h for h in head if h[0] not in ("map", "overflow")]
    assert fixed[0] == ["npix", str(NPIX)] and fixed[1][0] == "angle_deg" and float(fixed[1][1]) == ANGLE
    assert fixed[2][0] == "min_peak" and float(fixed[2][1]) == min_peak and len(fixed[2]) == 2
    assert fixed[3] == ["capacity", str(capacity)]
    assert fixed[-1] == ["z", *lead_names, "row", "col", "value", "dy", "dx", "off_row_deg", "off_col_deg", "flags"]
    names = [h[0] for h in fixed[4:-1]]
    assert ("smooth" in names) == ("smooth" in family) and ("sigma_e" in names) == ("noisy" in family)
    table = np.loadtxt(path, ndmin=2)
    if table.size == 0:
        table = np.zeros((0, 9 + len(lead_names)))
    want, want_maps, overflows = [], [], []
    for z in ZS:
        for prefix, lead in maps:
            rows, total = expected_rows(load_map(out, prefix, z), z, lead, min_peak, capacity)
            want.append(rows)
            label = [repr(float(z))] + [str(v) for v in lead]
            want_maps.append(label + ["n_peaks", str(total), "stored", str(len(rows))])
            if total > len(rows):
                overflows.append(label + [str(total - len(rows)), "peaks", "are", "not", "listed"])
    want = np.concatenate(want)
    got_maps = [h[1:] for h in head if h[0] == "map"]
    assert [[repr(float(m[0]))] + m[1:] for m in got_maps] == want_maps
    got_over = [h[1:] for h in head if h[0] == "overflow"]
    assert [[repr(float(m[0]))] + m[1:] for m in got_over] == overflows
    assert table.shape == want.shape, (family, table.shape, want.shape)
    assert table.tobytes() == want.tobytes(), family  # every float parses back to its own bits, -0.0 included
    # the '# map' line of a map stands in front of that map's rows
    body = [ln for ln in lines if ln and (not ln.startswith("#") or ln.startswith("# map"))]
    at = 0
    for m in want_maps:
        assert body[at].startswith("# map ")
        at += 1 + int(m[-1])
    assert at == len(body)
    return sum(int(m[-3]) for m in want_maps), len(want)


def mid_threshold(out):
    """A threshold from the run's own kappa files that keeps some peaks of every family and drops others."""
    return float(np.percentile(np.concatenate([load_map(out, "kappa", z).ravel() for z in ZS]).astype(np.float64), 75.0))


def test_catalogue_files_match_the_restatement_of_the_kappa_files(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    r = run([ini] + BASE)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert not files(out, "catalogue_") and len(files(out, ".fits")) > 12
    mid = mid_threshold(out)
    all_peaks = {}
    for spec, min_peak, capacity in (("-inf", -np.inf, DEFAULT_CAPACITY), (f"{mid!r},500", mid, 500)):
        clear(out)
        r = run([ini] + BASE + ["--catalogue", spec])
        assert r.returncode == 0, r.stderr[-2000:]
        assert "above the capacity" not in r.stderr
        for family in FAMILIES:
            peaks, rows = check_family(out, family, min_peak, capacity)
            assert peaks == rows > 0
            all_peaks.setdefault(spec, {})[family] = peaks
        # plane, kappa, smoothed and noisy files are byte-identical with and without --catalogue
        assert {f: b for f, b in files(out, "").items() if "catalogue_" not in f} == without
        assert sorted(files(out, "catalogue_")) == sorted(os.path.basename(table_path(out, f)) for f in FAMILIES)
    everything, above = all_peaks.values()
    assert all(above[f] <= everything[f] for f in FAMILIES) and sum(above.values()) < sum(everything.values())  # the threshold drops some


def test_a_capacity_of_one_is_announced_and_the_run_goes_on(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    r = run([ini] + BASE + ["--catalogue", "-inf,1"])
    assert r.returncode == 0, r.stderr[-2000:]
    n_maps = 0
    for family, (_, maps) in FAMILIES.items():
        peaks, rows = check_family(out, family, -np.inf, 1)
        assert rows == len(ZS) * len(maps) and peaks > 4 * rows
        assert open(table_path(out, family)).read().count("# overflow ") == rows
        n_maps += rows
    assert r.stderr.count("above the capacity: the first 1 are listed") == n_maps


def test_catalogue_files_are_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=NPIX)
    args = [ini, "--accum", "fixed64"] + BASE[1:] + ["--catalogue", "0.0"]
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    for family in FAMILIES:
        check_family(out, family, 0.0, DEFAULT_CAPACITY)
    one = files(out, "catalogue_")
    assert len(one) == len(FAMILIES)
    # resume: the kappa files and some plane files removed, the other planes read back; the tables are rewritten
    for f in files(out, "kappa_z"):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    for f in one:
        with open(os.path.join(out, f), "w") as fh:
            fh.write("stale\n")
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert files(out, "catalogue_") == one
    clear(out)
    for f in one:
        os.remove(os.path.join(out, f))
    r = run(args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, "catalogue_") == one


@pytest.mark.parametrize("args", [
    ["--catalogue", "0.0"],                            # without --kappa
    ["--kappa", "all", "--catalogue"],
    ["--kappa", "all", "--catalogue", ""],
    ["--kappa", "all", "--catalogue", "nan"],
    ["--kappa", "all", "--catalogue", "x"],
    ["--kappa", "all", "--catalogue", "0.0,"],
    ["--kappa", "all", "--catalogue", "0.0,0"],        # a capacity outside 1 ... 2^29
    ["--kappa", "all", "--catalogue", "0.0,536870913"],
    ["--kappa", "all", "--catalogue", "0.0,1.5"],
    ["--kappa", "all", "--catalogue", "0.0,8,2"],
])
def test_catalogue_is_refused_before_any_plane(tmp_path, args):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--catalogue" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or "catalogue_" in f]
