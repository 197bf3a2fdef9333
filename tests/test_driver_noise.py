"""SLICER_amd --kappa ... --shape-noise sigma_e,ngal[,seed[,nreal]]: the noisy maps written by the driver (DESIGN.md S8
row N13) against the Python API on the kappa files of the same run, bit for bit; their smoothed maps against Smooth of
them; the four tables against the restatements tests/moments_np.py and tests/peaks_np.py applied to those files; and
that nothing else changes."""
import os

import numpy as np
import pytest

import moments_np as M
import peaks_np as P
import slicer_amd
from test_driver import make_cone, run
from test_driver_shear import files, read_fits
from test_driver_smooth import cards, sigma_pix

pytestmark = pytest.mark.gpu

ANGLE = 2.0  # make_cone's field of view
LD = np.longdouble
SIGMA_E, NGAL, SEED, NREAL = 0.26, 30.0, 12345678901234567, 2
LO, HI, BINS = -0.03, 0.03, 8  # the noise of a pixel is 0.0127 (npix 32) and 0.0119 (npix 30)
LEVELS = 2
NOISE_KEYS = ["SIGMAE", "NGAL", "SIGMAPIX", "SEED", "REALIS"]


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


def noise_arg(seed=SEED, nreal=NREAL):
    return ["--shape-noise", f"{SIGMA_E!r},{NGAL!r},{seed},{nreal}"]


def key15(v):
    """v as a FITS key holds it: 15 significant digits."""
    return float("%.15G" % v)


def noise_lines(head, sp, seed=SEED):
    """The five '#' lines of --shape-noise, names and values."""
    assert [h[0] for h in head] == ["sigma_e", "ngal_arcmin2", "noise_sigma_pix", "seed", "nreal"] and all(len(h) == 2 for h in head)
    assert [float(h[1]) for h in head[:3]] == [SIGMA_E, NGAL, sp] and [int(h[1]) for h in head[3:]] == [seed, NREAL]


def not_noisy(out):
    return {f: b for f, b in files(out, "").items() if ".noisy" not in f}


def kappa_files(out):
    """{"%.4f" % z: path}, in ascending redshift."""
    found = {f[len("cone_gadget.kappa_z"):].split("_")[0]: os.path.join(out, f) for f in files(out, "cone_gadget.kappa_z")}
    return dict(sorted(found.items(), key=lambda kv: float(kv[0])))


def check_noisy_fits(slicer, out, npix, seed, kind, scales):
    """Every noisy file is the Python API on the run's own kappa file, every smoothed noisy file Smooth of that;
    -> ({(r, z): map}, {(r, k, z): map})."""
    sp = slicer_amd.noise_sigma_pix(SIGMA_E, NGAL, ANGLE, npix)
    kappa = kappa_files(out)
    assert len(kappa) == 2
    noisy, smoothed = {}, {}
    with slicer_amd.Noise(slicer, npix, seed) as nz:
        for stream, (z, kpath) in enumerate(kappa.items()):  # the stream: the source's rank in ascending redshift
            khead, x = read_fits(kpath, npix)
            d = slicer.to_device(x)
            try:
                for r in range(NREAL):
                    nz.run(d, sp, stream, r)
                    want = nz.read()
                    head, y = read_fits(os.path.join(out, f"cone_gadget.noisy{r}_kappa_z{z}_{npix}_t0.fits"), npix)
                    assert y.tobytes() == want.tobytes(), (r, z)
                    assert 0.5 * sp < float((y - x).std()) < 1.5 * sp
                    got = cards(head)
                    assert got[:-5] == cards(khead) and [c[0] for c in got[-5:]] == NOISE_KEYS
                    assert [float(c[1]) for c in got[-5:-2]] == [SIGMA_E, NGAL, key15(sp)] and int(got[-2][1]) == seed
                    assert int(got[-1][1]) == r
                    noisy[(r, z)] = y
                    for k, a in enumerate(scales):
                        with slicer_amd.Smooth(slicer, npix, kind, sigma_pix(a, npix)) as sm:
                            sm.run(nz.device_map())
                            want, R = sm.read(), sm.radius
                        name = f"cone_gadget.noisy{r}_{kind}{k}_kappa_z{z}_{npix}_t0.fits"
                        shead, ys = read_fits(os.path.join(out, name), npix)
                        assert ys.tobytes() == want.tobytes(), name
                        more = cards(shead)
                        assert more[:-3] == got and [c[0] for c in more[-3:]] == ["SCALE", "RADIUS", "NOISESIG"]
                        assert float(more[-3][1]) == a and int(more[-2][1]) == R
                        assert float(more[-1][1]) == key15(sp * slicer_amd.smooth_noise_gain(kind, sigma_pix(a, npix)))
                        smoothed[(r, k, z)] = ys
            finally:
                slicer.free(d)
    n_fits = [f for f in os.listdir(out) if ".noisy" in f and f.endswith(".fits")]
    assert len(n_fits) == len(noisy) + len(smoothed)
    return noisy, smoothed


def check_tables(out, token, npix, blocks, lead_names, n_head_moments, n_head_peaks, edges):
    """The moments and peaks tables `token` against the restatements: blocks = [(lead values, z, map)] in file order.
    -> the '#' lines of the moments table between the three first and the column names."""
    mom = os.path.join(out, f"cone_gadget.{token}moments_{npix}_t0.txt")
    pk = os.path.join(out, f"cone_gadget.{token}peaks_{npix}_t0.txt")
    hm = [ln[1:].split() for ln in open(mom) if ln.startswith("#")]
    hp = [ln[1:].split() for ln in open(pk) if ln.startswith("#")]
    assert hm[0] == hp[0] == ["npix", str(npix)] and hm[2] == hp[2] == ["levels", str(LEVELS)]
    assert hm[-1] == lead_names + ["z", "level", "npix", "mean"] + [f"S{k}" for k in M.ORDERS]
    assert hp[-1] == lead_names + ["z", "level", "npix", "bin", "lo", "hi", "n_pixels", "n_peaks", "n_minima"]
    assert len(hm) == 3 + n_head_moments + 1 and len(hp) == 4 + n_head_peaks + 1 and hm[3:-1] == hp[4:-1]
    tm, tp = np.loadtxt(mom, ndmin=2), np.loadtxt(pk, ndmin=2)
    q, B = len(lead_names), len(edges) - 1
    per = B + 3
    assert tm.shape == (len(blocks) * (LEVELS + 1), q + 11) and tp.shape == (tm.shape[0] * per, q + 9)
    row_at = 0
    for lead, z, x0 in blocks:
        for l, x in enumerate(M.pyramid(x0, LEVELS, "mean")):
            n = x.shape[0]
            row = tm[row_at]
            assert tuple(row[:q]) == tuple(lead) and f"{row[q]:.4f}" == z and row[q + 1] == l and row[q + 2] == n == npix >> l
            mean, mean_abs = M.mean_ld(x)
            assert abs(LD(row[q + 3]) - mean) <= M.mean_bound(mean_abs, n), (lead, z, l)
            ref, A = M.sums_ld(x, row[q + 3])
            assert np.all(np.abs(row[q + 4:].astype(LD) - ref) <= M.sum_bounds(A, n)), (lead, z, l)
            rows = tp[row_at * per:(row_at + 1) * per]
            assert np.all(rows[:, :q] == np.array(lead)) and np.all(rows[:, q] == row[q]) and np.all(rows[:, q + 1] == l)
            assert np.all(rows[:, q + 2] == n) and np.array_equal(rows[:, q + 3], np.arange(-1, B + 2))
            ref = P.counts(x, edges)
            for col, name, w in ((q + 6, "pdf", 0), (q + 7, "peaks", 1), (q + 8, "minima", 2)):
                want = [ref["below"][w]] + list(ref[name]) + [ref["above"][w]] + [ref["nan"] if w == 0 else 0]
                assert np.array_equal(rows[:, col].astype(np.int64), np.array(want, np.int64)), (lead, z, l, name)
            row_at += 1
    assert row_at == tm.shape[0]
    return hm[3:-1]


@pytest.mark.parametrize("npix,kind,scales", [(32, "gauss", (1.125, 5.625)), (30, "map", (3.0,))])
def test_noisy_files_and_tables(slicer, tmp_path, npix, kind, scales):
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--moments", "--moments-levels", str(LEVELS), "--peaks", f"{LO!r},{HI!r},{BINS}",
            "--smooth", kind + ":" + ",".join(repr(a) for a in scales)]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not any(".noisy" in f for f in without)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + noise_arg())
    assert r.returncode == 0, r.stderr[-2000:]
    # every pre-existing file is byte-identical with and without --shape-noise
    assert not_noisy(out) == without
    noisy, smoothed = check_noisy_fits(slicer, out, npix, SEED, kind, scales)
    edges = P.uniform_edges(LO, HI, BINS)
    zs = list(kappa_files(out))
    sp = slicer_amd.noise_sigma_pix(SIGMA_E, NGAL, ANGLE, npix)
    head = check_tables(out, "noisy_", npix, [((r,), z, noisy[(r, z)]) for z in zs for r in range(NREAL)], ["real"], 5, 5, edges)
    noise_lines(head, sp)
    blocks = [((r, k), z, smoothed[(r, k, z)]) for z in zs for r in range(NREAL) for k in range(len(scales))]
    head = check_tables(out, "noisy_smooth_", npix, blocks, ["real", "scale"], 10, 10, edges)
    assert head[0] == ["smooth", kind]
    noise_lines(head[4:9], sp)
    gains = [sp * slicer_amd.smooth_noise_gain(kind, sigma_pix(a, npix)) for a in scales]
    assert head[9][0] == "noise_sigma" and [float(v) for v in head[9][1:]] == gains
    # the smoothed noise has about that sigma: the maps are noise-dominated, the edges renormalised (gauss) or cropped
    for (r, k, z), y in smoothed.items():
        R = int(4.0 * sigma_pix(scales[k], npix) + 0.5)
        inner = y[R:npix - R, R:npix - R]
        if inner.size >= 100:
            assert 0.4 * gains[k] < float(inner.std()) < 2.0 * gains[k], (r, k, z)
    # another seed changes the noisy files and nothing else
    first = {f: b for f, b in files(out, ".noisy").items()}
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + noise_arg(seed=SEED + 1))
    assert r.returncode == 0, r.stderr[-2000:]
    assert not_noisy(out) == without
    second = files(out, ".noisy")
    assert sorted(second) == sorted(first) and all(second[f] != first[f] for f in first)


def test_noisy_outputs_are_the_same_resumed_on_two_ranks_and_with_the_sources_reordered(tmp_path):
    ini, _, out = make_cone(tmp_path)
    tail = ["--moments", "--moments-levels", "1", "--peaks", f"{LO!r},{HI!r},{BINS}", "--smooth", "map:1.875"] + noise_arg()
    args = [ini, "--accum", "fixed64", "--kappa", "0.05,0.2"] + tail
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = files(out, ".noisy")
    assert len(one) == 2 * NREAL * 2 + 4 and len([f for f in one if f.endswith(".txt")]) == 4
    everything = files(out, "")
    # resume: some plane files removed, the others read back; a map file that exists is never overwritten, so the kappa
    # files and what was made from them are removed
    for f in list(files(out, "kappa_z")):
        os.remove(os.path.join(out, f))
    for f in sorted(f for f in os.listdir(out) if ".plane_" in f)[1::3]:
        os.remove(os.path.join(out, f))
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert files(out, "") == everything
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert files(out, ".noisy") == one
    # the sources the other way round: the streams go with the redshifts, so every map file is the same (the tables list
    # the sources in the order given)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run([ini, "--accum", "fixed64", "--kappa", "0.2,0.05"] + tail)
    assert r.returncode == 0, r.stderr[-2000:]
    fits = lambda d: {f: b for f, b in d.items() if f.endswith(".fits")}
    assert fits(files(out, ".noisy")) == fits(one)
    assert fits(files(out, "")) == fits(everything)


@pytest.mark.parametrize("npix,args", [
    (32, ["--shape-noise", "0.26,30"]),                                  # without --kappa
    (32, ["--kappa", "all", "--shape-noise"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,1,2,3"]),
    (32, ["--kappa", "all", "--shape-noise", "0,30"]),
    (32, ["--kappa", "all", "--shape-noise", "-0.26,30"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,0"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,inf"]),
    (32, ["--kappa", "all", "--shape-noise", "nan,30"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,,1"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,x"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,-1"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,9223372036854775808"]),  # the SEED key is a signed 64-bit integer
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,1,0"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,1,1025"]),
    (32, ["--kappa", "all", "--shape-noise", "0.26,30,1,2.5"]),
    (-150, ["--kappa", "all", "--shape-noise", "0.26,30"]),              # a physical pixel size: no angle
])
def test_shape_noise_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--shape-noise" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or f.endswith(".txt")]
