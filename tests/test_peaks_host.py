"""The PDF-histogram and peak-count contract without a device: the restatement tests/peaks_np.py
against a plain double loop and against np.histogram, the peak and minimum fractions of white noise, the uniform edges
of slicer_peaks_edges against the stated formula, and the refusals of slicer_peaks_* that need no device."""
import ctypes as C

import numpy as np
import pytest

import peaks_np as P
import slicer_amd
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6


def _err():
    return (L.slicer_last_error(None) or b"").decode()


def loop_counts(x, edges):
    """The contract, one pixel and one edge at a time."""
    n, B = x.shape[0], len(edges) - 1
    out = {"pdf": [0] * B, "peaks": [0] * B, "minima": [0] * B, "below": [0] * 3, "above": [0] * 3, "nan": 0}

    def put(kind, name, v):
        v = float(v)  # f32 -> f64, exact
        if v < edges[0]:
            out["below"][kind] += 1
        elif v > edges[B]:
            out["above"][kind] += 1
        elif v == edges[B]:
            out[name][B - 1] += 1
        else:
            for b in range(B):
                if edges[b] <= v < edges[b + 1]:
                    out[name][b] += 1

    for i in range(n):
        for j in range(n):
            v = x[i, j]
            if np.isnan(v):
                out["nan"] += 1
                continue
            put(0, "pdf", v)
            if not (1 <= i <= n - 2 and 1 <= j <= n - 2):
                continue
            nb = [x[i + di, j + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)]
            if all(v > w for w in nb):
                put(1, "peaks", v)
            if all(v < w for w in nb):
                put(2, "minima", v)
    return out


def same(got, ref):
    return all(np.array_equal(np.asarray(got[k], np.int64), np.asarray(ref[k], np.int64))
               for k in ("pdf", "peaks", "minima", "below", "above", "nan"))


@pytest.mark.parametrize("n", range(1, 10))
def test_restatement_against_a_plain_loop(n):
    rng = np.random.default_rng(100 + n)
    ties = rng.integers(-3, 4, (n, n)).astype(np.float32)
    smooth = rng.standard_normal((n, n)).astype(np.float32)
    holes = smooth.copy()
    holes.ravel()[::5] = np.nan
    holes.ravel()[1::7] = np.inf
    holes.ravel()[2::11] = -np.inf
    for x in (ties, smooth, holes):
        for edges in (np.array([-2.0, 2.0]), P.uniform_edges(-2, 2, 8), np.array([-2.5, -1.0, 0.0, 0.125, 3.0])):
            got = P.counts(x, edges)
            assert same(got, loop_counts(x, [float(e) for e in edges])), (n, edges)
            assert got["pdf"].sum() + got["below"][0] + got["above"][0] + got["nan"] == n * n
    if n < 3:
        assert P.counts(smooth, [-9.0, 9.0])["peaks"].sum() == 0 == P.counts(smooth, [-9.0, 9.0])["minima"].sum()


def test_pdf_is_np_histogram_on_data_inside_the_edges():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (200, 200)).astype(np.float32)
    x[0, :5] = [-1.0, 1.0, 0.0, 0.5, -0.5]  # on the edges, the closed last one included
    for edges in (P.uniform_edges(-1, 1, 64), P.uniform_edges(-1, 1, 7), np.array([-1.0, -0.9, 0.0, 0.001, 1.0])):
        got = P.counts(x, edges)
        assert np.array_equal(got["pdf"], np.histogram(x.astype(np.float64), edges)[0])
        assert got["below"][0] == got["above"][0] == got["nan"] == 0


@pytest.mark.parametrize("n", [64, 257, 1000])
def test_a_ninth_of_white_noise_is_a_peak_and_a_ninth_a_minimum(n):
    # the centre of 9 exchangeable values is the largest with probability 1/9; adjacent pixels cannot both be peaks, so
    # the counts are negatively correlated and the binomial width is conservative
    x = np.random.default_rng(7919 * n).standard_normal((n, n)).astype(np.float32)
    peak, minimum = P.extrema(x)
    N, p = (n - 2) ** 2, 1.0 / 9.0
    sigma = np.sqrt(p * (1 - p) / N)
    for mask in (peak, minimum):
        print(f"n {n}: (fraction - 1/9) / sigma = {(mask.sum() / N - p) / sigma:.3f}")
        assert abs(mask.sum() / N - p) <= 5 * sigma
    assert not (peak & minimum).any()
    got = P.counts(x, P.uniform_edges(-5, 5, 64), (peak, minimum))
    assert got["peaks"].sum() + got["below"][1] + got["above"][1] == peak.sum()
    assert got["peaks"][:32].sum() < got["peaks"][32:].sum() and got["minima"][:32].sum() > got["minima"][32:].sum()


@pytest.mark.parametrize("lo,hi,bins", [(-0.05, 0.3, 1024), (-5.0, 5.0, 64), (0.1, 0.7, 7), (-1.0, 2.0, 1), (1e-3, 1.0, 3),
                                        (-1e300, 1e300, 1024)])
def test_uniform_edges_are_the_formula(lo, hi, bins):
    got = slicer_amd.peaks_edges(lo, hi, bins)
    assert got.dtype == np.float64 and got.shape == (bins + 1,)
    width = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
    ref = [np.float64(lo)] + [np.float64(lo) + np.float64(b) * width for b in range(1, bins)] + [np.float64(hi)]
    assert got.tobytes() == np.array(ref, np.float64).tobytes()
    assert got.tobytes() == P.uniform_edges(lo, hi, bins).tobytes()
    assert np.all(np.diff(got) > 0)
    e = np.zeros(bins + 1)
    assert L.slicer_peaks_edges(lo, hi, bins, e.ctypes.data) == 0 and e.tobytes() == got.tobytes()


@pytest.mark.parametrize("lo,hi,bins,text", [
    (0.0, 1.0, 0, "bins = 0 outside 1..1024"),
    (0.0, 1.0, -2, "bins = -2 outside 1..1024"),
    (0.0, 1.0, 1025, "bins = 1025 outside 1..1024"),
    (np.nan, 1.0, 4, "lo and hi must be finite"),
    (0.0, np.inf, 4, "lo and hi must be finite"),
    (1.0, 1.0, 4, None),
    (2.0, 1.0, 4, None),
    (1.0, 1.0 + 2.0 ** -50, 1024, None),  # four doubles between the two: no room for 1023 distinct edges
    (-1.7e308, 1.7e308, 2, None),  # hi - lo overflows
])
def test_uniform_edges_refusals(lo, hi, bins, text):
    e = np.zeros(1100)
    assert L.slicer_peaks_edges(lo, hi, bins, e.ctypes.data) == ERR_ARG
    if text is None:
        text = "the edges of lo = %.17g, hi = %.17g, bins = %d are not finite and strictly ascending" % (lo, hi, bins)
    assert _err() == "slicer_peaks_edges: " + text
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.peaks_edges(lo, hi, bins)


def test_uniform_edges_refuse_a_null_array():
    assert L.slicer_peaks_edges(0.0, 1.0, 4, None) == ERR_ARG
    assert _err() == "slicer_peaks_edges: null argument"


@pytest.mark.parametrize("npix,edges,code,text", [
    (0, [0.0, 1.0], ERR_ARG, "npix must be positive"),
    (-4, [0.0, 1.0], ERR_ARG, "npix must be positive"),
    (131073, [0.0, 1.0], ERR_UNSUPPORTED, "npix = 131073 above 131072"),
    (16, [0.0], ERR_ARG, "fewer than 2 edges"),
    (16, [], ERR_ARG, "fewer than 2 edges"),
    (16, list(range(1026)), ERR_ARG, "1026 edges, at most 1025"),
    (16, [0.0, np.nan, 1.0], ERR_ARG, "edges must be finite"),
    (16, [0.0, 1.0, np.inf], ERR_ARG, "edges must be finite"),
    (16, [-np.inf, 0.0, 1.0], ERR_ARG, "edges must be finite"),
    (16, [0.0, 1.0, 1.0], ERR_ARG, "edges must be strictly ascending"),
    (16, [0.0, 2.0, 1.0], ERR_ARG, "edges must be strictly ascending"),
    (16, [0.0, 1.0], ERR_ARG, "null argument"),
    (131072, list(range(1025)), ERR_ARG, "null argument"),
])
def test_create_refusals_need_no_device(npix, edges, code, text):
    e = np.array(edges, np.float64)
    out = C.c_void_p(1)
    assert L.slicer_peaks_create(None, npix, e.size, e.ctypes.data, C.byref(out)) == code
    assert _err() == "slicer_peaks_create: " + text
    assert not out.value
    assert L.slicer_peaks_create(None, npix, e.size, e.ctypes.data, None) == code


def test_create_refuses_null_edges():
    out = C.c_void_p(1)
    assert L.slicer_peaks_create(None, 16, 3, None, C.byref(out)) == ERR_ARG
    assert _err() == "slicer_peaks_create: null argument"
    assert not out.value


def test_calls_without_a_handle():
    buf = np.zeros(8, np.int64)
    assert L.slicer_peaks_run(None, buf.ctypes.data) == ERR_ARG
    assert _err() == "slicer_peaks_run: null argument"
    assert L.slicer_peaks_run_npix(None, buf.ctypes.data, 1) == ERR_ARG
    assert _err() == "slicer_peaks_run_npix: null argument"
    assert L.slicer_peaks_read(None, buf.ctypes.data, None, None, None, None, None) == ERR_ARG
    assert _err() == "slicer_peaks_read: null handle"
    assert L.slicer_peaks_destroy(None) == ERR_ARG
