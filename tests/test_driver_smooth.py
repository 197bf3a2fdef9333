"""SLICER_amd --kappa ... --smooth gauss|map:a1,a2,...: the smoothed maps written by the driver
against the Python API on the kappa files of the same run, bit for bit, and the two tables of the smoothed maps against
the restatements tests/moments_np.py and tests/peaks_np.py applied to the smoothed files."""
import os

import numpy as np
import pytest

import moments_np as M
import peaks_np as P
import slicer_amd
from test_driver import make_cone, run
from test_driver_peaks import choose_range, spec
from test_driver_shear import clear, files, read_fits

pytestmark = pytest.mark.gpu

ANGLE = 2.0  # make_cone's field of view
LD = np.longdouble
BINS = 8
OTHERS = (".kappa_z", ".plane_", ".moments_", ".peaks_", ".gamma1_z", ".phi_z", ".cl_")
SMOOTHED = (".gauss", ".map", ".smooth_moments_", ".smooth_peaks_")


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


def sigma_pix(a, npix):
    return a * npix / (60.0 * ANGLE)


def cards(header):
    """[(name, value text)] of a FITS header block up to END."""
    out = []
    for k in range(0, len(header), 80):
        card = header[k:k + 80].decode()
        if card.startswith("END"):
            break
        out.append((card[:8].strip(), card[10:30].strip()))
    return out


def smoothed_files(out, kind, npix):
    """{(k, "%.4f" % z): path} of the run's smoothed files."""
    found = {}
    for f in sorted(os.listdir(out)):
        if f.startswith(f"cone_gadget.{kind}") and "_kappa_z" in f:
            k, rest = f[len(f"cone_gadget.{kind}"):].split("_kappa_z")
            assert rest.endswith(f"_{npix}_t0.fits")
            found[(int(k), rest.split("_")[0])] = os.path.join(out, f)
    return found


def check_fits(slicer, out, npix, kind, scales):
    """Every smoothed file is the Python API on the run's own kappa file; -> {(k, z): map}."""
    found = smoothed_files(out, kind, npix)
    kappa = {f[len("cone_gadget.kappa_z"):].split("_")[0]: os.path.join(out, f) for f in files(out, ".kappa_z")}
    assert len(kappa) == 2 and sorted(found) == sorted((k, z) for k in range(len(scales)) for z in kappa)
    maps = {}
    for (k, z), path in found.items():
        khead, x = read_fits(kappa[z], npix)
        head, y = read_fits(path, npix)
        d = slicer.to_device(x)
        try:
            with slicer_amd.Smooth(slicer, npix, kind, sigma_pix(scales[k], npix)) as sm:
                sm.run(d)
                want, R = sm.read(), sm.radius
        finally:
            slicer.free(d)
        assert y.tobytes() == want.tobytes(), (kind, k, z)
        assert float(np.abs(y).max()) > 0
        got = cards(head)
        assert got[:-2] == cards(khead) and [c[0] for c in got[-2:]] == ["SCALE", "RADIUS"]
        assert float(got[-2][1]) == scales[k] and int(got[-1][1]) == R == int(4.0 * sigma_pix(scales[k], npix) + 0.5)
        maps[(k, z)] = y
    return maps


def check_head(path, npix, levels, kind, scales, n_before):
    head = [ln[1:].split() for ln in open(path) if ln.startswith("#")]
    assert head[0] == ["npix", str(npix)] and head[1][0] == "angle_deg" and head[2] == ["levels", str(levels)]
    h = head[n_before:]
    assert h[0] == ["smooth", kind]
    assert h[1][0] == "scales_arcmin" and [float(v) for v in h[1][1:]] == list(scales)
    assert h[2][0] == "sigma_pix" and [float(v) for v in h[2][1:]] == [sigma_pix(a, npix) for a in scales]
    assert h[3][0] == "radius" and [int(v) for v in h[3][1:]] == [int(4.0 * sigma_pix(a, npix) + 0.5) for a in scales]
    assert len(h) == 5
    return h[4]


def check_tables(out, npix, levels, kind, scales, maps, edges):
    """The two tables against the restatements of the smoothed files' pyramids."""
    mom = os.path.join(out, f"cone_gadget.smooth_moments_{npix}_t0.txt")
    pk = os.path.join(out, f"cone_gadget.smooth_peaks_{npix}_t0.txt")
    assert check_head(mom, npix, levels, kind, scales, 3) == ["scale", "z", "level", "npix", "mean"] + [f"S{k}" for k in M.ORDERS]
    assert check_head(pk, npix, levels, kind, scales, 4) == ["scale", "z", "level", "npix", "bin", "lo", "hi", "n_pixels",
                                                            "n_peaks", "n_minima"]
    tm, tp = np.loadtxt(mom, ndmin=2), np.loadtxt(pk, ndmin=2)
    B = len(edges) - 1
    per = B + 3
    assert tm.shape == (len(maps) * (levels + 1), 12) and tp.shape == (len(maps) * (levels + 1) * per, 10)
    zs = sorted({z for _, z in maps}, key=float)
    block = 0
    for z in zs:  # per source, scale by scale
        for k in range(len(scales)):
            pyr = M.pyramid(maps[(k, z)], levels, "mean")
            for l, x in enumerate(pyr):
                n = x.shape[0]
                row = tm[block]
                assert row[0] == k and f"{row[1]:.4f}" == z and row[2] == l and row[3] == n == npix >> l
                mean, mean_abs = M.mean_ld(x)
                assert abs(LD(row[4]) - mean) <= M.mean_bound(mean_abs, n), (z, k, l)
                ref, A = M.sums_ld(x, row[4])
                assert np.all(np.abs(row[5:].astype(LD) - ref) <= M.sum_bounds(A, n)), (z, k, l)
                rows = tp[block * per:(block + 1) * per]
                assert np.all(rows[:, 0] == k) and np.all(rows[:, 1] == row[1]) and np.all(rows[:, 2] == l)
                assert np.all(rows[:, 3] == n) and np.array_equal(rows[:, 4], np.arange(-1, B + 2))
                assert rows[1:-1, 5].tobytes() == edges.tobytes() and rows[:-2, 6].tobytes() == edges.tobytes()
                ref = P.counts(x, edges)
                for col, name, q in ((7, "pdf", 0), (8, "peaks", 1), (9, "minima", 2)):
                    want = [ref["below"][q]] + list(ref[name]) + [ref["above"][q]] + [ref["nan"] if q == 0 else 0]
                    assert np.array_equal(rows[:, col].astype(np.int64), np.array(want, np.int64)), (z, k, l, name)
                assert rows[:, 7].sum() == n * n
                block += 1
    assert block == tm.shape[0]


# the scales give R = 1 and 6 (gauss) and 2 or 3 (map) at truncate 4
@pytest.mark.parametrize("npix,kind,scales", [(32, "gauss", (1.125, 5.625)), (32, "map", (2.8125,)),
                                              (30, "gauss", (2.0, 6.0)), (30, "map", (3.0,))])
def test_smoothed_files_and_tables(slicer, tmp_path, npix, kind, scales):
    ini, _, out = make_cone(tmp_path, npix=npix)
    levels = 2
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--shear", "--power", "auto", "--moments", "--moments-levels", str(levels)]
    smooth = ["--smooth", kind + ":" + ",".join(repr(a) for a in scales)]
    # without --peaks: the smoothed files and the moments table of the smoothed maps alone
    r = run(base + smooth)
    assert r.returncode == 0, r.stderr[-2000:]
    first = {key: y.tobytes() for key, y in check_fits(slicer, out, npix, kind, scales).items()}
    assert len(files(out, ".smooth_moments_")) == 1 and not files(out, ".smooth_peaks_") and not files(out, ".peaks_")
    lo, hi = choose_range(out, npix)
    peaks = ["--peaks", spec(lo, hi, BINS)]
    clear(out)
    os.remove(os.path.join(out, f"cone_gadget.smooth_moments_{npix}_t0.txt"))
    r = run(base + peaks)
    assert r.returncode == 0, r.stderr[-2000:]
    without = {k: files(out, k) for k in OTHERS}
    assert all(without[k] for k in OTHERS) and not any(files(out, k) for k in SMOOTHED)
    clear(out)
    r = run(base + peaks + smooth)
    assert r.returncode == 0, r.stderr[-2000:]
    maps = check_fits(slicer, out, npix, kind, scales)
    assert {key: y.tobytes() for key, y in maps.items()} == first
    check_tables(out, npix, levels, kind, scales, maps, P.uniform_edges(lo, hi, BINS))
    # every other file is byte-identical with and without --smooth (no smoothed file's name holds one of these tokens)
    assert {k: files(out, k) for k in OTHERS} == without


def test_smoothed_outputs_are_the_same_resumed_and_on_two_ranks(tmp_path):
    ini, _, out = make_cone(tmp_path)
    base = [ini, "--accum", "fixed64", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "2"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    lo, hi = choose_range(out, 32)
    args = base + ["--peaks", spec(lo, hi, BINS), "--smooth", "map:1.875,2.8125"]
    clear(out)
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    kinds = ("map0_kappa_z", "map1_kappa_z", ".smooth_moments_", ".smooth_peaks_", ".moments_", ".peaks_")
    one = {k: files(out, k) for k in kinds}
    assert [len(one[k]) for k in kinds] == [2, 2, 1, 1, 1, 1]
    # resume: some plane files removed, the others read back; the tables are left in place and rewritten (a map file
    # that exists is never overwritten, so the kappa files and the smoothed ones are removed)
    for f in list(files(out, "kappa_z")):
        os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert {k: files(out, k) for k in kinds} == one
    clear(out)
    for f in [f for f in os.listdir(out) if f.endswith(".txt")]:
        os.remove(os.path.join(out, f))
    r = run(args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert {k: files(out, k) for k in kinds} == one


@pytest.mark.parametrize("args", [
    ["--smooth", "gauss:2"],                              # without --kappa
    ["--kappa", "all", "--smooth", "tophat:2"],           # a bad kind
    ["--kappa", "all", "--smooth", "gauss"],
    ["--kappa", "all", "--smooth", "2,3"],
    ["--kappa", "all", "--smooth", "gauss:"],             # an empty or negative scale, a bad list
    ["--kappa", "all", "--smooth", "gauss:2,,3"],
    ["--kappa", "all", "--smooth", "map:-2"],
    ["--kappa", "all", "--smooth", "map:2,0"],
    ["--kappa", "all", "--smooth", "map:2,x"],
    ["--kappa", "all", "--smooth", "map:2,inf"],
    ["--kappa", "all", "--smooth"],
    ["--kappa", "all", "--smooth", "gauss:2,0.4"],        # sigma = 0.107 pixels: R = 0
    ["--kappa", "all", "--smooth", "map:2,121"],          # sigma = 32.3 pixels: R = 129
])
def test_smooth_is_refused_before_any_plane(tmp_path, args):
    ini, _, out = make_cone(tmp_path)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--smooth" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or f.endswith(".txt")]
