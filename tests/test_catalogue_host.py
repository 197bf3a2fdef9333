"""The peak / minimum catalogue without a device: the numpy restatement tests/catalogue_np.py
against an independent least-squares fit, against an exact quadratic, class by class of the refinement's outcomes and
against the counts of tests/peaks_np.py (row N10); what slicer_catalogue_* refuses before it looks at a handle; and the
record's layout against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import catalogue_np as K
import peaks_np as P
from slicer_amd import _lib, lensing

L = lensing._L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 2, 6
MAX_NPIX, MAX_CAPACITY = 32768, 1 << 29


def _err():
    return (L.slicer_last_error(None) or b"").decode()


# ---- the refinement ------------------------------------------------------------------------------
def test_the_fit_is_the_least_squares_quadratic():
    """z(a, b) = c + gy a + gx b + hyy a^2 / 2 + hxy a b + hxx b^2 / 2 fitted to the nine points by numpy.linalg.lstsq.
    Bound: both sides round a handful of f64 operations on values of the window's size, and the design matrix is well
    conditioned (its columns are orthogonal but for 1 and a^2, b^2): 1e-12 of the window's largest |z| is four decades
    above that."""
    a, b = (v.ravel().astype(np.float64) for v in np.meshgrid([-1, 0, 1], [-1, 0, 1], indexing="ij"))
    design = np.stack([np.ones(9), a, b, a * a / 2, a * b, b * b / 2], axis=1)
    rng = np.random.default_rng(22)
    for scale in (1.0, 1e-3, 1e4):
        z = (rng.standard_normal((200, 3, 3)) * scale).astype(np.float32).astype(np.float64)
        gy, gx, hyy, hxx, hxy = K.window_terms(z)
        for k in range(len(z)):
            c = np.linalg.lstsq(design, z[k].ravel(), rcond=None)[0]
            got = np.array([gy[k], gx[k], hyy[k], hxy[k], hxx[k]])
            assert np.all(np.abs(got - c[1:]) <= 1e-12 * np.abs(z[k]).max()), (k, got, c)


def quadratic(n, centre, oy, ox, sign=1.0):
    """An exact quadratic in f32 (every coefficient and offset a small dyadic number) with its extremum at centre + (oy, ox)."""
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    u, v = i - (centre[0] + oy), j - (centre[1] + ox)
    f = sign * (8.0 - u * u - 0.5 * u * v - 2.0 * v * v)
    assert np.array_equal(f.astype(np.float32).astype(np.float64), f)
    return f.astype(np.float32)


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("oy,ox", [(0.25, -0.125), (-0.375, 0.4375), (0.0, 0.0), (0.4375, -0.25), (0.0625, 0.0)])
def test_an_exact_quadratic_gives_its_offset_back(sign, oy, ox):
    x = quadratic(7, (3, 3), oy, ox, sign)
    rec = K.catalogue(x, K.PEAKS if sign > 0 else K.MINIMA)
    assert len(rec) == 1 and (rec["row"][0], rec["col"][0]) == (3, 3)
    assert rec["flags"][0] == (0 if sign > 0 else K.MINIMUM) and rec["value"][0] == x[3, 3]
    assert abs(rec["dy"][0] - oy) <= 1e-12 and abs(rec["dx"][0] - ox) <= 1e-12
    assert len(K.catalogue(x, K.MINIMA if sign > 0 else K.PEAKS)) == 0


def centred(window):
    """A 5 x 5 map with `window` (3 x 3) about (2, 2) and the centre's value on the rim: every other interior pixel
    touches the rim, so none of them is an extremum of the centre's kind."""
    x = np.full((5, 5), np.float32(window[1][1]), np.float32)
    x[1:4, 1:4] = np.asarray(window, np.float32)
    return x


INF, NAN = np.inf, np.nan
KIND = {1.0: K.PEAKS, -1.0: K.MINIMA}
# name: (window of a would-be peak at its centre, the records expected, refine's reason)
CLASSES = {
    "accepted": (quadratic(3, (1, 1), 0.25, -0.125), 1, 0),
    "det": ([[-0.9, 0, 0.9], [0, 1, 0], [0.9, 0, -0.9]], 1, 1),
    "hyy": ([[0.9, -10, 0.9], [-10, 1, -10], [0.9, -10, 0.9]], 1, 2),
    # -a^2 - (b - 0.9)^2 with its centre raised from -0.81 to just above its right neighbour: the fit's maximum is 0.71 to the right
    "far": ([[-4.61, -1.81, -1.01], [-3.61, 0.0, -0.01], [-4.61, -1.81, -1.01]], 1, 4),
    "inf": ([[0, 0, 0], [0, 1, -INF], [0, 0, 0]], 1, None),
    "nan": ([[0, 0, 0], [0, 1, NAN], [0, 0, 0]], 0, None),
    "tie": ([[0, 0, 0], [0, 1, 1], [0, 0, 0]], 0, None),
}


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_every_class_of_the_refinement_is_met(sign):
    seen = set()
    for name, (window, n_rec, reason) in CLASSES.items():
        x = centred(sign * np.asarray(window, np.float64))
        rec, why = K.catalogue(x, KIND[sign], with_why=True)
        at_centre = rec[(rec["row"] == 2) & (rec["col"] == 2)]
        assert len(rec) == len(at_centre) == n_rec, (name, rec)
        if not n_rec:
            seen.add(name)
            continue
        r = at_centre[0]
        assert bool(r["flags"] & K.MINIMUM) == (sign < 0) and r["value"] == x[2, 2]
        if name == "accepted":
            assert not r["flags"] & K.FALLBACK and abs(r["dy"] - 0.25) <= 1e-12 and abs(r["dx"] + 0.125) <= 1e-12
        else:
            assert r["flags"] & K.FALLBACK
            assert r["dy"] == 0.0 and r["dx"] == 0.0 and not np.signbit(r["dy"]) and not np.signbit(r["dx"])
        if reason is not None:
            assert why[0] == reason, (name, why)
        else:
            assert np.isinf(x).any() and why[0] != 0
        seen.add(name)
    assert seen == set(CLASSES)
    # the classes are told apart by the first rule that fails: each one is met
    reasons = {K.catalogue(centred(sign * np.asarray(w, np.float64)), KIND[sign], with_why=True)[1][0]
               for w, n, _ in CLASSES.values() if n}
    assert {0, 1, 2, 4} <= reasons


def test_a_negative_zero_offset_is_kept():
    """dy = -(0 / det) is -0.0 where the gradient vanishes: the restatement keeps the sign, and so must the device."""
    x = quadratic(5, (2, 2), 0.0, 0.0)
    rec = K.catalogue(x, K.PEAKS)
    assert len(rec) == 1 and rec["flags"][0] == 0 and rec["dy"][0] == 0.0 and np.signbit(rec["dy"][0]) and np.signbit(rec["dx"][0])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 17, 64, 129])
def test_the_records_are_the_extrema_that_peaks_counts(n):
    rng = np.random.default_rng(n)
    edges = P.uniform_edges(-1.0, 1.0, 7)
    for x in (rng.standard_normal((n, n)).astype(np.float32), rng.integers(-3, 4, (n, n)).astype(np.float32)):
        ref = P.counts(x, edges)
        rec = K.catalogue(x)
        peaks, minima = K.totals(rec)
        assert peaks == ref["peaks"].sum() + ref["below"][1] + ref["above"][1]
        assert minima == ref["minima"].sum() + ref["below"][2] + ref["above"][2]
        key = rec["row"].astype(np.int64) * n + rec["col"]
        assert np.all(np.diff(key) > 0)
        assert len(K.catalogue(x, K.PEAKS)) == peaks and len(K.catalogue(x, K.MINIMA)) == minima
        # the thresholds are closed: a threshold on a record's own value keeps it
        if peaks:
            v = np.float64(rec["value"][~(rec["flags"] & 1).astype(bool)].max())
            assert len(K.catalogue(x, K.PEAKS, min_peak=v)) >= 1
            assert len(K.catalogue(x, K.PEAKS, min_peak=np.nextafter(v, np.inf))) == 0


# ---- refusals that need no device ----------------------------------------------------------------
def test_create_refuses_its_numbers_before_the_handle():
    who = "slicer_catalogue_create: "
    cases = [((0, 16, None), ERR_ARG, who + "npix must be positive"),
             ((MAX_NPIX + 1, 16, None), ERR_UNSUPPORTED, who + f"npix = {MAX_NPIX + 1} above {MAX_NPIX}"),
             ((16, 0, None), ERR_ARG, who + f"capacity = 0 outside 1..{MAX_CAPACITY}"),
             ((16, MAX_CAPACITY + 1, None), ERR_ARG, who + f"capacity = {MAX_CAPACITY + 1} outside 1..{MAX_CAPACITY}"),
             ((16, 16, 8), ERR_ARG, who + "the records are off the 16-byte grid"),
             ((MAX_NPIX, MAX_CAPACITY, None), ERR_ARG, who + "null argument")]  # numbers that are taken: the handle is missed
    for args, code, text in cases:
        out = C.c_void_p(1)
        assert L.slicer_catalogue_create(None, *args, C.byref(out)) == code, args
        assert _err() == text
        assert out.value is None
    assert L.slicer_catalogue_create(None, 16, 16, None, None) == ERR_ARG  # a null out
    assert _err() == who + "null argument"
    assert L.slicer_catalogue_create(None, 0, 16, None, None) == ERR_ARG  # ... after the numbers
    assert _err() == who + "npix must be positive"


@pytest.mark.parametrize("name,tail", [("slicer_catalogue_run", ()), ("slicer_catalogue_run_npix", (16,))])
def test_run_refuses_its_selection_before_the_handle(name, tail):
    run = getattr(L, name)
    buf = np.zeros(4, np.float32)
    for kinds in (0, 4, -1):
        assert run(None, buf.ctypes.data, kinds, 0.0, 0.0, *tail) == ERR_ARG
        assert _err() == f"{name}: kinds = {kinds} outside 1..3"
    for lo, hi in ((np.nan, 0.0), (0.0, np.nan), (np.nan, np.nan)):
        assert run(None, buf.ctypes.data, 3, lo, hi, *tail) == ERR_ARG
        assert _err() == f"{name}: a threshold is NaN"
    for lo, hi in ((-np.inf, np.inf), (np.inf, -np.inf), (0.5, 0.25)):  # infinite thresholds are taken: now the handle is missed
        assert run(None, buf.ctypes.data, 1, lo, hi, *tail) == ERR_ARG
        assert _err() == f"{name}: null argument"


def test_the_other_entry_points_without_a_handle():
    for name, args in (("count", (None, None, None)), ("read", (None, 0, None)), ("device", (None, None))):
        assert getattr(L, f"slicer_catalogue_{name}")(None, *args) == ERR_ARG
        assert _err() == f"slicer_catalogue_{name}: null handle"
    assert L.slicer_catalogue_destroy(None) == ERR_ARG


# ---- the record ----------------------------------------------------------------------------------
def test_record_layout_matches_header(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "slicer_amd.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(slicer_catalogue_record), offsetof(slicer_catalogue_record, row),
         offsetof(slicer_catalogue_record, col), offsetof(slicer_catalogue_record, value),
         offsetof(slicer_catalogue_record, flags), offsetof(slicer_catalogue_record, dy), offsetof(slicer_catalogue_record, dx));
  printf("%d %d %u %u %d %d\n", SLICER_CATALOGUE_PEAKS, SLICER_CATALOGUE_MINIMA, SLICER_CATALOGUE_MINIMUM,
         SLICER_CATALOGUE_FALLBACK, SLICER_CATALOGUE_MAX_NPIX, SLICER_CATALOGUE_MAX_CAPACITY);
  return 0; }''')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    R = _lib.CatalogueRecord
    fields = ("row", "col", "value", "flags", "dy", "dx")
    assert [int(v) for v in out[0].split()] == [32, 0, 4, 8, 12, 16, 24]
    assert [int(v) for v in out[0].split()] == [C.sizeof(R)] + [getattr(R, f).offset for f in fields]
    for dt in (lensing.CATALOGUE_DTYPE, K.DTYPE):
        assert [int(v) for v in out[0].split()] == [dt.itemsize] + [dt.fields[f][1] for f in fields]
        assert dt.names == fields
    assert [np.dtype(lensing.CATALOGUE_DTYPE.fields[f][0]) for f in fields] == [np.dtype(K.DTYPE.fields[f][0]) for f in fields]
    assert [int(v) for v in out[1].split()] == [lensing.CATALOGUE_PEAKS, lensing.CATALOGUE_MINIMA, lensing.CATALOGUE_MINIMUM,
                                                lensing.CATALOGUE_FALLBACK, lensing.CATALOGUE_MAX_NPIX,
                                                lensing.CATALOGUE_MAX_CAPACITY]
    assert (K.PEAKS, K.MINIMA, K.MINIMUM, K.FALLBACK) == (1, 2, 1, 2)
