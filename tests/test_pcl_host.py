"""Host-side checks of the masked pseudo-C_l: the two routes of the restatement in
tests/pcl_np.py to the coupling matrix, the taper table of slicer_pcl_taper, and the FITS image reader of the driver's
--pcl-mask.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import pcl_np
import slicer_amd
from slicer_amd import fits


def hole_mask(n):
    """A 3-pixel taper times a rectangular hole."""
    user = np.ones((n, n), np.float32)
    user[n // 3:n // 3 + 3, n // 2:n // 2 + 4] = 0.0
    return pcl_np.mask(n, 3.0, user)


@pytest.mark.parametrize("n", [12, 15, 16])
def test_restatement_routes_agree(n):
    edges = [0, 1, 2, 3.5, 5, 0.75 * n]
    w = hole_mask(n)
    fft, brute = pcl_np.coupling_fft(w, edges), pcl_np.coupling_brute(w, edges)
    assert float(np.abs(fft - brute).max()) <= 1e-14


@pytest.mark.parametrize("n", [12, 16])
def test_restatement_constant_mask(n):
    edges = [0, 1, 2, 3.5, 5, 0.75 * n]
    for c in (1.0, 0.5):
        M = pcl_np.coupling_brute(np.full((n, n), c), edges)
        assert float(np.abs(M - c * c * np.eye(5)).max()) <= 1e-14


@pytest.mark.parametrize("n,width", [(2, 1.0), (12, 3.0), (15, 3.0), (45, 9.0), (128, 25.6), (128, 1000.0), (49, 0.25),
                                      (4096, 64.0)])
def test_taper_table(n, width):
    f = slicer_amd.pcl_taper(n, width)
    ref = pcl_np.taper(n, width)
    assert float((np.abs(f - ref) / np.spacing(ref)).max()) <= 2.0
    i = np.arange(n)
    t = (np.minimum(i, n - 1 - i) + 0.5) / width
    assert np.all(f[t >= 1.0] == 1.0)
    assert np.all((f > 0.0) & (f <= 1.0))
    assert np.array_equal(f, f[::-1])


def test_taper_refusals():
    for n, width in ((1, 3.0), (0, 3.0), (-4, 3.0), (16, 0.0), (16, -1.0), (16, float("inf")), (16, float("nan"))):
        with pytest.raises(slicer_amd.SlicerError) as e:
            slicer_amd.pcl_taper(n, width)
        assert e.value.code == 2, (n, width)  # SLICER_ERR_ARG


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READER = os.path.join(ROOT, "tests", "cpp", "fits_read_driver")


def read_back(path, n):
    r = subprocess.run([READER, str(path), str(n)], capture_output=True)
    return r.returncode, np.frombuffer(r.stdout, np.float32), r.stderr.decode()


@pytest.mark.parametrize("n", [1, 7, 30])
def test_mask_reader_reads_what_write_image_wrote(tmp_path, n):
    """The reader behind SLICER_amd --pcl-mask, through tests/cpp/fits_read_driver."""
    assert os.path.exists(READER), "run __graft_entry__.build()"
    rng = np.random.default_rng(n)
    image = rng.standard_normal((n, n))
    image[0, 0] = 1e-300  # rounds to 0 in f32
    image[-1, -1] = 1 + 2.0 ** -30
    keys = [("ANGLE", 2.0, " "), ("nparttype3", 7, " ")]
    for bitpix, given in ((-32, image.astype(np.float32)), (-64, image)):
        path = tmp_path / f"image{bitpix}.fits"
        fits.write_image(str(path), given, keys, bitpix=bitpix)
        rc, got, _ = read_back(path, n)
        assert rc == 0
        assert np.array_equal(got.view(np.uint32), given.astype(np.float32).ravel().view(np.uint32))
        # another shape than the file's
        rc, got, why = read_back(path, n + 1)
        assert rc == 1 and got.size == 0 and "not an image of" in why


def test_mask_reader_refusals(tmp_path):
    n = 6
    good = tmp_path / "good.fits"
    fits.write_image(str(good), np.ones((n, n), np.float32), [])
    raw = good.read_bytes()

    def refused(name, data, text):
        path = tmp_path / name
        path.write_bytes(data)
        rc, got, why = read_back(path, n)
        assert rc == 1 and got.size == 0 and text in why, (name, why)
    for bitpix in (16, 32, 8, 64):
        card = ("BITPIX  = %20d" % bitpix).encode()
        refused(f"bitpix{bitpix}.fits", raw.replace(b"BITPIX  =                  -32", card), "BITPIX")
    refused("cube.fits", raw.replace(b"NAXIS   =                    2", b"NAXIS   =                    3"), "not an image of")
    refused("wide.fits", raw.replace(b"NAXIS1  = %20d" % n, b"NAXIS1  = %20d" % (n + 1)), "not an image of")
    refused("short.fits", raw[:2880 + 4 * n * n - 1], "shorter")
    refused("text.fits", b"not a FITS file\n" * 400, "not a FITS file")
    refused("scaled.fits", raw.replace(b"EXTEND  =                    T", b"BZERO   =                32768"), "BSCALE")
    rc, got, why = read_back(tmp_path / "missing.fits", n)
    assert rc == 1 and "cannot open" in why
