"""SLICER_amd --kappa ... --starlet J:lo,hi,bins: the starlet maps written by the driver against
slicer_amd.Starlet on the kappa files of the same run, bit for bit; the two tables against tests/peaks_np.py and the l1
restatement of tests/starlet_np.py applied to those files; with --shape-noise the signal-to-noise edges and the noisy
realisations; and that nothing else changes."""
import os

import numpy as np
import pytest

import peaks_np as P
import slicer_amd
import starlet_np as W
from test_driver import make_cone, run
from test_driver_noise import ANGLE, NGAL, NREAL, SIGMA_E, kappa_files, noise_arg, noise_lines
from test_driver_shear import files, read_fits

pytestmark = pytest.mark.gpu

J = 3
BINS = 8


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


def cards(header):
    """[(name, value text)] of a FITS header block up to END; the value is what stands between "= " and " /"."""
    out = []
    for k in range(0, len(header), 80):
        card = header[k:k + 80].decode()
        if card.startswith("END"):
            break
        out.append((card[:8].strip(), card[10:].split(" /")[0].strip()))
    return out


def not_starlet(out):
    return {f: b for f, b in files(out, "").items() if "starlet" not in f}


def check_fits(slicer, out, npix, sources, prefix):
    """Every <prefix>starlet<j> file is slicer_amd.Starlet on the file `sources[z]` of the same run, with its header and
    the cards SCALE and GAIN; -> {(z, j): map}."""
    gains, coarse = slicer_amd.starlet_gains(J)
    gain = [coarse] + list(gains)
    maps = {}
    with slicer_amd.Starlet(slicer, npix, J) as st:
        for z, path in sources.items():
            khead, x = read_fits(path, npix)
            d = slicer.to_device(x)
            try:
                st.run(d)
                want = st.read_all()
            finally:
                slicer.free(d)
            ref = W.starlet(x, J)
            for j in range(J + 1):
                name = f"cone_gadget.{prefix}starlet{j}_kappa_z{z}_{npix}_t0.fits"
                head, y = read_fits(os.path.join(out, name), npix)
                assert y.tobytes() == want[j].tobytes(), name
                assert np.array_equal(y, ref[j])  # (finite maps: the restatement's values)
                got = cards(head)
                assert got[:-2] == cards(khead) and [c[0] for c in got[-2:]] == ["SCALE", "GAIN"]
                assert int(got[-2][1]) == j and got[-1][1] == "%.17g" % gain[j] and float(got[-1][1]) == gain[j]
                maps[(z, j)] = y
    return maps


def check_tables(out, token, npix, blocks, lead_names, edges_of, n_noise_lines):
    """The tables <token>starlet_peaks_ and <token>starlet_l1_: blocks = [(lead values, z, {j: map})] in file order,
    edges_of(j) the edges of scale j; -> the '#' lines between the fifth and the column names."""
    pk = os.path.join(out, f"cone_gadget.{token}starlet_peaks_{npix}_t0.txt")
    l1 = os.path.join(out, f"cone_gadget.{token}starlet_l1_{npix}_t0.txt")
    hp = [ln[1:].split() for ln in open(pk) if ln.startswith("#")]
    hl = [ln[1:].split() for ln in open(l1) if ln.startswith("#")]
    assert hp[:-1] == hl[:-1] and len(hp) == 5 + n_noise_lines + 1
    assert hp[0] == ["npix", str(npix)] and float(hp[1][1]) == ANGLE and hp[2] == ["scales", str(J)]
    assert hp[3][0] == "edges" and hp[4][0] == "gain"
    assert [float(v) for v in hp[4][1:]] == list(slicer_amd.starlet_gains(J)[0])
    assert hp[-1] == lead_names + ["z", "scale", "bin", "edge_lo", "edge_hi", "n_pixels", "n_peaks", "n_minima"]
    assert hl[-1] == lead_names + ["z", "scale", "bin", "edge_lo", "edge_hi", "count", "l1"]
    tp, tl = np.loadtxt(pk, ndmin=2), np.loadtxt(l1, ndmin=2)
    q, per = len(lead_names), BINS + 3
    assert tp.shape == (len(blocks) * J * per, q + 8) and tl.shape == (len(blocks) * J * per, q + 7)
    at = 0
    for lead, z, maps in blocks:
        for j in range(1, J + 1):
            e = edges_of(j)
            rp, rl = tp[at:at + per], tl[at:at + per]
            for rows in (rp, rl):
                assert np.all(rows[:, :q] == np.array(lead)) and all(f"{v:.4f}" == z for v in rows[:, q])
                assert np.all(rows[:, q + 1] == j) and np.array_equal(rows[:, q + 2], np.arange(-1, BINS + 2))
                assert np.array_equal(rows[1:-2, q + 3], e[:-1]) and np.array_equal(rows[1:-2, q + 4], e[1:])
                assert rows[0, q + 4] == e[0] and rows[-2, q + 3] == e[-1]
            ref = P.counts(maps[j], e)
            for col, name, w in ((q + 5, "pdf", 0), (q + 6, "peaks", 1), (q + 7, "minima", 2)):
                want = [ref["below"][w]] + list(ref[name]) + [ref["above"][w]] + [ref["nan"] if w == 0 else 0]
                assert np.array_equal(rp[:, col].astype(np.int64), np.array(want, np.int64)), (lead, z, j, name)
            ref = W.l1norm(maps[j], e)
            counts = np.array([ref["below"]] + list(ref["counts"]) + [ref["above"], ref["nan"]], np.float64)
            exact = np.array([ref["below_l1"]] + list(ref["l1"]) + [ref["above_l1"], 0.0])
            assert np.array_equal(rl[:, q + 5], counts), (lead, z, j)
            assert (np.abs(rl[:, q + 6] - exact) <= counts * 2.0 ** -53 * exact).all(), (lead, z, j)
            assert counts[:-1].sum() == npix * npix and counts[1:-2].sum() > 0
            at += per
    assert at == tp.shape[0]
    return hp[5:-1]


@pytest.mark.parametrize("npix", [32, 30])
def test_starlet_files_and_tables(slicer, tmp_path, npix):
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--peaks", "-0.03,0.03,4"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 8 and not any("starlet" in f for f in without)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    lo, hi = -0.004, 0.006
    r = run(base + ["--starlet", f"{J}:{lo!r},{hi!r},{BINS}"])
    assert r.returncode == 0, r.stderr[-2000:]
    # every other file is byte-identical with and without --starlet
    assert not_starlet(out) == without
    kappa = kappa_files(out)
    assert len(kappa) == 2
    maps = check_fits(slicer, out, npix, kappa, "")
    assert sorted(f for f in files(out, "starlet") if f.endswith(".fits")) == sorted(
        f"cone_gadget.starlet{j}_kappa_z{z}_{npix}_t0.fits" for z in kappa for j in range(J + 1))
    assert len([f for f in files(out, "starlet") if f.endswith(".txt")]) == 2
    edges = slicer_amd.peaks_edges(lo, hi, BINS)
    blocks = [((), z, {j: maps[(z, j)] for j in range(1, J + 1)}) for z in kappa]
    head = check_tables(out, "", npix, blocks, [], lambda j: edges, 0)
    assert head == []
    hp = [ln[1:].split() for ln in open(os.path.join(out, f"cone_gadget.starlet_l1_{npix}_t0.txt")) if ln.startswith("#")]
    assert [float(v) for v in hp[3][1:]] == list(edges)


def test_starlet_with_shape_noise_is_in_units_of_each_scales_noise(slicer, tmp_path):
    npix = 32
    ini, _, out = make_cone(tmp_path, npix=npix)
    lo, hi = -3.0, 5.0
    r = run([ini, "--ngp", "--kappa", "0.05,0.2", "--starlet", f"{J}:{lo!r},{hi!r},{BINS}"] + noise_arg())
    assert r.returncode == 0, r.stderr[-2000:]
    sp = slicer_amd.noise_sigma_pix(SIGMA_E, NGAL, ANGLE, npix)
    sigma = [sp * g for g in slicer_amd.starlet_gains(J)[0]]          # sigma_j = RN(sigma_pix gain_j)
    unit = slicer_amd.peaks_edges(lo, hi, BINS)
    edges_of = lambda j: unit * sigma[j - 1]                          # e_jb = RN(e_b sigma_j)
    kappa = kappa_files(out)
    clean = check_fits(slicer, out, npix, kappa, "")
    blocks = [((), z, {j: clean[(z, j)] for j in range(1, J + 1)}) for z in kappa]
    head = check_tables(out, "", npix, blocks, [], edges_of, 6)
    noise_lines(head[:5], sp)
    assert head[5][0] == "sigma_scale" and [float(v) for v in head[5][1:]] == sigma
    # the noisy realisations: the same maps and tables of the noisy files
    blocks = []
    for z in kappa:
        for real in range(NREAL):
            noisy = {z: os.path.join(out, f"cone_gadget.noisy{real}_kappa_z{z}_{npix}_t0.fits")}
            maps = check_fits(slicer, out, npix, noisy, f"noisy{real}_")
            blocks.append(((real,), z, {j: maps[(z, j)] for j in range(1, J + 1)}))
            # the transform is linear: what the noise added to scale j has about the rms sigma_j.  An rms over about
            # (npix / 2^j)^2 independent values, 16 at j = 3, scatters by 1 / sqrt(2 * 16) = 18 %: +-3.3 of those
            for j in range(1, J + 1):
                added = maps[(z, j)].astype(np.float64) - clean[(z, j)]
                assert 0.4 * sigma[j - 1] < float(added.std()) < 1.6 * sigma[j - 1], (z, real, j)
    head = check_tables(out, "noisy_", npix, blocks, ["real"], edges_of, 6)
    noise_lines(head[:5], sp)
    n_fits = [f for f in files(out, "starlet") if f.endswith(".fits")]
    assert len(n_fits) == len(kappa) * (J + 1) * (1 + NREAL) and len(files(out, "starlet")) == len(n_fits) + 4


@pytest.mark.parametrize("npix,args", [
    (32, ["--starlet", "3:-1,1,8"]),                                  # without --kappa
    (32, ["--kappa", "all", "--starlet"]),
    (32, ["--kappa", "all", "--starlet", "3"]),
    (32, ["--kappa", "all", "--starlet", "0:-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "13:-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "-2:-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "2.5:-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "x:-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", ":-1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "3:-1,1"]),
    (32, ["--kappa", "all", "--starlet", "3:1,1,8"]),
    (32, ["--kappa", "all", "--starlet", "3:1,-1,8"]),
    (32, ["--kappa", "all", "--starlet", "3:-1,inf,8"]),
    (32, ["--kappa", "all", "--starlet", "3:-1,1,0"]),
    (32, ["--kappa", "all", "--starlet", "3:-1,1,1025"]),
    (32, ["--kappa", "all", "--starlet", "3:-1,1,8,9"]),
    (-150, ["--kappa", "all", "--starlet", "3:-1,1,8"]),              # a physical pixel size: no angle
])
def test_starlet_is_refused_before_any_plane(tmp_path, npix, args):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert "--starlet" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or f.endswith(".txt")]
