"""SLICER_amd with every statistic of the kappa maps at once (--moments, --peaks, --minkowski over the plain, the
smoothed, the noisy and the smoothed noisy maps, --power, --bispectrum): which files it writes, in which order it
announces them on stdout, and the '#' lines of the twelve tables.  All expected text is written out here as one run
left it; the numbers inside the tables are those of test_driver_{moments,peaks,minkowski,smooth,noise}.py."""
import os

import pytest

from test_driver import make_cone, run

ARGS = ["--ngp", "--kappa", "all", "--moments", "--moments-levels", "2", "--peaks", "-0.02,0.08,8", "--minkowski",
        "-0.02,0.08,8", "--smooth", "gauss:4,8", "--shape-noise", "0.3,30,7,2", "--power", "cross", "--bispectrum",
        "equilateral", "--bispectrum-edges", "1,4,8,12"]

ZS = ["0.0084", "0.0167", "0.0252", "0.0336", "0.0421", "0.0506", "0.0592", "0.0678", "0.0764", "0.0850", "0.0937",
      "0.1025", "0.1113", "0.1201", "0.1289", "0.1378", "0.1467", "0.1557", "0.1647", "0.1738", "0.1829", "0.1920",
      "0.2012"]
# per source, in this order: what stdout calls the map, and its file token
SOURCE_MAPS = [("convergence", ".kappa_z"),
               ("smoothed convergence", ".gauss0_kappa_z"),
               ("smoothed convergence", ".gauss1_kappa_z"),
               ("noisy convergence", ".noisy0_kappa_z"),
               ("smoothed noisy convergence", ".noisy0_gauss0_kappa_z"),
               ("smoothed noisy convergence", ".noisy0_gauss1_kappa_z"),
               ("noisy convergence", ".noisy1_kappa_z"),
               ("smoothed noisy convergence", ".noisy1_gauss0_kappa_z"),
               ("smoothed noisy convergence", ".noisy1_gauss1_kappa_z")]
# after the sources, in this order
TABLES = [("power spectra", ".cl_"),
          ("bispectra", ".bl_"),
          ("moments", ".moments_"),
          ("histograms and peak counts", ".peaks_"),
          ("moments of the smoothed maps", ".smooth_moments_"),
          ("histograms and peak counts of the smoothed maps", ".smooth_peaks_"),
          ("moments of the noisy maps", ".noisy_moments_"),
          ("histograms and peak counts of the noisy maps", ".noisy_peaks_"),
          ("moments of the smoothed noisy maps", ".noisy_smooth_moments_"),
          ("histograms and peak counts of the smoothed noisy maps", ".noisy_smooth_peaks_"),
          ("Minkowski functionals", ".minkowski_"),
          ("Minkowski functionals of the smoothed maps", ".smooth_minkowski_"),
          ("Minkowski functionals of the noisy maps", ".noisy_minkowski_"),
          ("Minkowski functionals of the smoothed noisy maps", ".noisy_smooth_minkowski_")]

TOP = "# npix 30\n# angle_deg 2\n# levels 2\n"
VALUES = (" -0.02 -0.0074999999999999997 0.005000000000000001 0.017500000000000005 0.030000000000000002"
          " 0.042499999999999996 0.055000000000000007 0.067500000000000004 0.080000000000000002\n")
SMOOTH = "# smooth gauss\n# scales_arcmin 4 8\n# sigma_pix 1 2\n# radius 4 8\n"
NOISE = "# sigma_e 0.29999999999999999\n# ngal_arcmin2 30\n# noise_sigma_pix 0.013693063937629152\n# seed 7\n# nreal 2\n"
NOISE_SIGMA = "# noise_sigma 0.0038631646332450489 0.0019314389345705867\n"
COLUMNS = {"moments": "z level npix mean S2 S3 S4 S5 S6 S7 S8\n",
           "peaks": "z level npix bin lo hi n_pixels n_peaks n_minima\n",
           "minkowski": "z level npix j threshold n_faces n_edges n_vertices n_boundary n_border euler n_nan\n"}
VALUE_LINE = {"moments": "", "peaks": "# edges" + VALUES, "minkowski": "# thresholds" + VALUES}
# infix of the file name: the '#' lines between the statistic's own and the column names, the leading column names
KINDS = {"": ("", ""),
         "smooth_": (SMOOTH, "scale "),
         "noisy_": (NOISE, "real "),
         "noisy_smooth_": (SMOOTH + NOISE + NOISE_SIGMA, "real scale ")}


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    ini, _, out = make_cone(tmp_path_factory.mktemp("tables"), npix=30)
    r = run([ini] + ARGS)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, out


@pytest.mark.gpu
def test_the_files_are_exactly_the_expected_ones(full_run):
    _, out = full_run
    expected = {"cone_planes_list_t0.txt"}
    expected |= {f"cone_gadget.{i:03d}.plane_30_t0.fits" for i in range(23)}
    expected |= {f"cone_gadget{token}{z}_30_t0.fits" for z in ZS for _, token in SOURCE_MAPS}
    expected |= {f"cone_gadget{token}30_t0.txt" for _, token in TABLES}
    assert len(expected) == 245
    assert set(os.listdir(out)) == expected


@pytest.mark.gpu
def test_stdout_announces_the_files_in_order(full_run):
    stdout, out = full_run
    said = [line for line in stdout.split("\n") if line.startswith("Saving the ")]
    where = os.path.join(out, "cone_gadget")
    expected = [f"Saving the maps on: {where}.{i:03d}.plane_30_t0.fits" for i in range(23)]
    expected += [f"Saving the {what} map on: {where}{token}{z}_30_t0.fits" for z in ZS for what, token in SOURCE_MAPS]
    expected += [f"Saving the {what} on: {where}{token}30_t0.txt" for what, token in TABLES]
    assert said == expected


@pytest.mark.gpu
@pytest.mark.parametrize("statistic", ["moments", "peaks", "minkowski"])
@pytest.mark.parametrize("infix", list(KINDS))
def test_table_headers(full_run, statistic, infix):
    _, out = full_run
    text = open(os.path.join(out, f"cone_gadget.{infix}{statistic}_30_t0.txt")).read()
    head, lead_names = KINDS[infix]
    expected = TOP + VALUE_LINE[statistic] + head + "# " + lead_names + COLUMNS[statistic]
    assert text.startswith(expected)
    assert not any(line.startswith("#") for line in text[len(expected):].split("\n"))


@pytest.mark.gpu
def test_spectra_headers(full_run):
    _, out = full_run
    for token, fourth in ((".cl_", None), (".bl_", "# ell_edges 180 720 1440 2160")):
        lines = open(os.path.join(out, f"cone_gadget{token}30_t0.txt")).read().split("\n")
        assert lines[:2] == ["# npix 30", "# angle_deg 2"]
        assert lines[2].startswith("# zs ") and len(lines[2].split()) == 2 + len(ZS)
        if fourth:
            assert lines[3] == fourth
            assert lines[4] == ("# i j k ell_mean_i ell_mean_j ell_mean_k n_triangles "
                                + " ".join(f"B_{s}" for s in range(len(ZS))))
