"""SLICER_amd --kappa ... --scattering J,L: the tables written by the driver against the restatement
of tests/scattering_np.py applied to the kappa files of the same run, and with --shape-noise to its noisy files; every
coefficient inside the device bound of tests/test_gpu_scattering.py."""
import math
import os

import numpy as np
import pytest

import scattering_np as SN
from test_driver import make_cone, run
from test_driver_peaks import ANGLE, kappa_maps
from test_driver_shear import files, read_fits

COLUMNS = ["z", "order", "j1", "l1", "j2", "l2", "value", "power"]


def table_file(out, npix, token=".scattering_"):
    return os.path.join(out, f"cone_gadget{token}{npix}_t0.txt")


def read_table(path, npix, J, L, lead=()):
    """The rows of a table after its '#' lines have been checked; `lead`: the names of the leading columns."""
    head = {ln[1:].split()[0]: ln[1:].split()[1:] for ln in open(path) if ln.startswith("#")}
    assert head["npix"] == [str(npix)] and float(head["angle_deg"][0]) == ANGLE
    assert head["J"] == [str(J)] and head["L"] == [str(L)]
    assert float(head["sigma0"][0]) == 0.8 and float(head["xi0"][0]) == 3.0 * math.pi / 4.0 and float(head["slant"][0]) == 4.0
    last = [ln[1:].split() for ln in open(path) if ln.startswith("#")][-1]
    assert last == list(lead) + COLUMNS
    table = np.loadtxt(path, ndmin=2)
    assert table.shape[1] == len(lead) + len(COLUMNS)
    return head, table


def saved_files(stdout):
    """The names of the files the run announced, in its order (the directory may have any name)."""
    return [os.path.basename(ln.split(" on: ")[1]) for ln in stdout.splitlines() if ln.startswith("Saving the ")]


def rows_per_source(J, L):
    return 1 + J * L + J * (J - 1) // 2 * L * L


def check_block(rows, kappa, J, L, z):
    """The rows of one map against the restatement of it; returns the largest error as a fraction of the bound."""
    assert rows.shape == (rows_per_source(J, L), len(COLUMNS)) and np.all(rows[:, 0] == z)
    ref = SN.coefficients(kappa, J, L)
    u = SN.unit(kappa)
    worst = 0.0
    k = 0

    def close(got, want):
        nonlocal worst
        bound = SN.device_bound(want, u)
        if bound > 0:
            worst = max(worst, abs(got - want) / bound)
        else:  # an empty map, in front of every plane
            assert got == want == 0.0

    assert list(rows[k, 1:6]) == [0, -1, -1, -1, -1]
    close(rows[k, 6], ref["s0"][0])
    close(rows[k, 7], ref["s0"][1])
    k += 1
    for j1 in range(J):
        for l1 in range(L):
            assert list(rows[k, 1:6]) == [1, j1, l1, -1, -1]
            close(rows[k, 6], ref["s1"][j1, l1])
            close(rows[k, 7], ref["p1"][j1, l1])
            k += 1
    for j1 in range(J):
        for l1 in range(L):
            for j2 in range(j1 + 1, J):
                for l2 in range(L):
                    assert list(rows[k, 1:6]) == [2, j1, l1, j2, l2] and np.isnan(rows[k, 7])
                    close(rows[k, 6], ref["s2"][j1, l1, j2, l2])
                    k += 1
    assert k == rows.shape[0] and worst <= 1.0, worst
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("npix,J,L", [(32, 3, 2), (30, 2, 3)])
def test_scattering_file_matches_the_restatement(tmp_path, npix, J, L):
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "all", "--peaks", "-0.01,0.05,8", "--power", "auto", "--betti", "-0.01,0.05,4"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not files(out, "scattering")
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + ["--scattering", f"{J},{L}"])
    assert r.returncode == 0, r.stderr[-2000:]
    # every other file is byte-identical with and without --scattering
    assert {f: b for f, b in files(out, "").items() if "scattering" not in f} == without
    assert list(files(out, "scattering")) == [os.path.basename(table_file(out, npix))]
    # the table is announced after every other file of the run, the Betti table included
    said = saved_files(r.stdout)
    assert "scattering_" in said[-1] and not any("scattering" in f for f in said[:-1])
    _, table = read_table(table_file(out, npix), npix, J, L)
    maps = kappa_maps(out, npix)
    n = rows_per_source(J, L)
    assert table.shape[0] == len(maps) * n and len(maps) >= 20
    assert np.count_nonzero(table[table[:, 1] == 2, 6] > 0) >= 20 * L  # the comparison is of something
    worst = 0.0
    for s in range(len(maps)):
        z = table[s * n, 0]
        worst = max(worst, check_block(table[s * n:(s + 1) * n], maps[f"{z:.4f}"], J, L, z))
    print(f"npix = {npix}: largest error / bound of the table {worst:.4f}")


@pytest.mark.gpu
def test_the_two_tables_with_shape_noise(tmp_path):
    npix, J, L = 30, 3, 2
    ini, _, out = make_cone(tmp_path, npix=npix)
    base = [ini, "--ngp", "--kappa", "0.05,0.2", "--moments", "--moments-levels", "1", "--smooth", "gauss:4",
            "--shape-noise", "0.3,30,7,2", "--peaks", "-0.01,0.05,8", "--betti", "-0.01,0.05,4"]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = files(out, "")
    assert len(without) > 20 and not files(out, "scattering")
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    r = run(base + ["--scattering", f"{J},{L}"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert {f: b for f, b in files(out, "").items() if "scattering" not in f} == without
    assert sorted(files(out, "scattering")) == sorted(os.path.basename(table_file(out, npix, k)) for k in (
        ".scattering_", ".noisy_scattering_"))  # none for the smoothed maps or the pyramid levels
    said = saved_files(r.stdout)
    assert all("scattering_" in f for f in said[-2:]) and not any("scattering" in f for f in said[:-2])
    zs = sorted(kappa_maps(out, npix))
    n = rows_per_source(J, L)
    _, table = read_table(table_file(out, npix), npix, J, L)
    assert table.shape[0] == len(zs) * n
    for s in range(len(zs)):
        z = table[s * n, 0]
        check_block(table[s * n:(s + 1) * n], kappa_maps(out, npix)[f"{z:.4f}"], J, L, z)
    head, noisy = read_table(table_file(out, npix, ".noisy_scattering_"), npix, J, L, ("real",))
    assert head["nreal"] == ["2"] and head["seed"] == ["7"]
    blocks = noisy.reshape(-1, n, noisy.shape[1])
    assert blocks.shape[0] == len(zs) * 2
    seen = set()
    for b in blocks:
        real, z = int(b[0, 0]), b[0, 1]
        assert np.all(b[:, 0] == real)
        seen.add((real, f"{z:.4f}"))
        x = read_fits(os.path.join(out, f"cone_gadget.noisy{real}_kappa_z{z:.4f}_{npix}_t0.fits"), npix)[1]
        check_block(b[:, 1:], x, J, L, z)
    assert len(seen) == blocks.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args,message", [
    (32, ["--scattering", "3,2"], "--scattering needs --kappa (the coefficients are those of the kappa maps)"),
    (32, ["--kappa", "all", "--scattering", "3"], "bad --scattering"),        # not two numbers
    (32, ["--kappa", "all", "--scattering", "3,2,1"], "bad --scattering"),
    (32, ["--kappa", "all", "--scattering", "0,2"], "bad --scattering"),      # J outside 1 ... 12
    (32, ["--kappa", "all", "--scattering", "13,2"], "bad --scattering"),
    (32, ["--kappa", "all", "--scattering", "3,17"], "bad --scattering"),     # L outside 1 ... 16
    (32, ["--kappa", "all", "--scattering", "3,x"], "bad --scattering"),
    (32, ["--kappa", "all", "--scattering"], "bad --scattering"),
    (32, ["--kappa", "all", "--scattering", "6,2"], "--scattering: 2^J = 64 is above npix = 32"),
    (33, ["--kappa", "all", "--scattering", "3,2"], "--scattering: npix = 33 is not supported"),
    (-150, ["--kappa", "all", "--scattering", "3,2"], "--scattering: the table is that of maps with an angle"),
])
def test_scattering_is_refused_before_any_plane(tmp_path, npix, args, message):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert message in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits") or "scattering" in f]
