"""SLICER_amd with every lensing output at once: the options share one host map buffer, one shear handle (--shear and
--raytrace) and the pyramid that --moments hands to --peaks, so every file of a run with all of them has to be, byte for
byte, the file that a run with only its own options writes."""
import os

import pytest

from test_driver import make_cone, run
from test_driver_shear import clear, files

KAPPA = ["--ngp", "--kappa", "0.05,0.1,0.2"]
SHEAR_POWER = ["--shear", "--deflection", "--power", "cross"]
MOMENTS_PEAKS = ["--moments", "--moments-levels", "2", "--peaks", "-0.05,0.2,16"]
RAYS = ["--raytrace"]
TABLES = (".cl_", ".moments_", ".peaks_")
PER_SOURCE = {"shear": (".phi_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".alpha1_z", ".alpha2_z"),
              "rays": (".rt_kappa_z", ".rt_gamma1_z", ".rt_gamma2_z", ".rt_omega_z", ".rt_alpha1_z", ".rt_alpha2_z")}


def written(ini, out, args):
    """{name: bytes} of every file in `out` after a run that started without maps and tables."""
    clear(out)
    for f in os.listdir(out):
        if any(t in f for t in TABLES):
            os.remove(os.path.join(out, f))
    r = run([ini] + KAPPA + args)
    assert r.returncode == 0, r.stderr[-2000:]
    return files(out, "")


def count(got, token):
    return sum(token in f for f in got)


@pytest.mark.gpu
def test_all_lensing_options_together_write_the_files_of_the_separate_runs(tmp_path):
    ini, _, out = make_cone(tmp_path)
    a = written(ini, out, SHEAR_POWER)
    b = written(ini, out, MOMENTS_PEAKS)
    c = written(ini, out, RAYS)
    d = written(ini, out, SHEAR_POWER + MOMENTS_PEAKS + RAYS)
    # the separate runs wrote what they were asked for, and only that
    for got, has in ((a, PER_SOURCE["shear"] + (".cl_",)), (b, (".moments_", ".peaks_")), (c, PER_SOURCE["rays"])):
        assert count(got, ".plane_") >= 20 and count(got, ".kappa_z") == 3
        for token in PER_SOURCE["shear"] + PER_SOURCE["rays"]:
            assert count(got, token) == (3 if token in has else 0), token
        for token in TABLES:
            assert count(got, token) == (1 if token in has else 0), token
    for name, got in (("shear and power", a), ("moments and peaks", b), ("rays", c)):
        for f, data in got.items():
            assert f in d, (name, f)
            assert d[f] == data, (name, f)
    assert sorted(d) == sorted(set(a) | set(b) | set(c))
