"""Return codes and exact slicer_last_error texts of the add-on modules (weights, kappa, shear, power): the refusals
that need no device work.  Messages of failed HIP calls carry a source position and are not pinned here."""
import ctypes as C

import numpy as np
import pytest

import slicer_amd
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 2, 3, 6
UNSMOOTH = "npix = 11 unsupported (2..16384, prime factors 2, 3, 5, 7 only)"


def _err(h=None):
    return (L.slicer_last_error(h) or b"").decode()


def _bins(npix, n_edges, edges):
    c = np.zeros(64, np.int64)
    m = np.zeros(64)
    e = None if edges is None else np.asarray(edges, np.float64)
    return L.slicer_power_bins(npix, n_edges, None if e is None else e.ctypes.data, c.ctypes.data, m.ctypes.data)


@pytest.mark.parametrize("npix,n_edges,edges,text", [
    (16, 1, [0.0], "fewer than 2 edges"),
    (16, 3, [3.0, 2.0, 1.0], "edges must be strictly ascending"),
    (16, 15, None, "n_edges must be npix for the default edges (edges = NULL)"),
])
def test_power_bins_refusals(npix, n_edges, edges, text):
    assert _bins(npix, n_edges, edges) == ERR_ARG
    assert _err() == "slicer_power_bins: " + text


def _create_calls(h, out):
    return [("slicer_kappa_create", lambda: L.slicer_kappa_create(h, 16, 1, out)),
            ("slicer_shear_create", lambda: L.slicer_shear_create(h, 16, 5.0, out)),
            ("slicer_power_create", lambda: L.slicer_power_create(h, 16, 5.0, 1, 0, 16, None, out))]


@pytest.mark.parametrize("null_out", [False, True])
def test_create_without_a_handle(null_out):
    out = C.c_void_p()
    for name, call in _create_calls(None, None if null_out else C.byref(out)):
        assert call() == ERR_ARG
        assert _err() == name + ": null argument"
        assert not out.value


def test_power_read_without_a_handle():
    assert L.slicer_power_read(None, None, None, None) == ERR_ARG
    assert _err() == "slicer_power_read: null handle"


def _weights(omega_m, omega_lambda, physical):
    ld, ld2, zsnap, coeff = np.array([0.0]), np.array([100.0]), np.array([0.1]), np.zeros(1)
    return L.slicer_lensing_weights(omega_m, omega_lambda, -1.0, 0.0, 5.0, 16, 0, physical, 1, ld.ctypes.data,
                                    ld2.ctypes.data, zsnap.ctypes.data, 1, None, coeff.ctypes.data, None, None, None,
                                    None)


def test_lensing_weights_refusals():
    assert _weights(0.3, 0.7, 1) == ERR_UNSUPPORTED
    assert _err() == "kappa maps: a physical pixel size (one map size per plane) is not supported"
    assert _weights(0.3, 0.6, 0) == ERR_UNSUPPORTED
    assert _err() == "kappa maps need a flat background (Omega_m = 0.3, Omega_Lambda = 0.6)"


# ---- with a handle ------------------------------------------------------------------------------
N = 16


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@pytest.mark.gpu
def test_create_with_a_null_out_pointer(slicer):
    for name, call in _create_calls(slicer._h, None):
        assert call() == ERR_ARG
        assert _err(slicer._h) == name + ": null argument"


@pytest.mark.gpu
def test_shear_create_refuses_an_unsmooth_size(slicer):
    out = C.c_void_p()
    assert L.slicer_shear_create(slicer._h, 11, 5.0, C.byref(out)) == ERR_UNSUPPORTED
    assert _err(slicer._h) == "slicer_shear_create: " + UNSMOOTH
    assert not out.value


@pytest.mark.gpu
@pytest.mark.parametrize("npix,angle,n_maps,cross,code,text", [
    (11, 5.0, 1, 0, ERR_UNSUPPORTED, UNSMOOTH),
    (N, 5.0, 129, 0, ERR_UNSUPPORTED, "n_maps = 129 outside 1..128"),
    (N, 5.0, 1, 2, ERR_ARG, "cross = 2, expected 0 or 1"),
    (N, 0.0, 1, 0, ERR_ARG, "the angle must be positive and finite"),
    (N, -5.0, 1, 0, ERR_ARG, "the angle must be positive and finite"),
])
def test_power_create_refusals(slicer, npix, angle, n_maps, cross, code, text):
    out = C.c_void_p()
    assert L.slicer_power_create(slicer._h, npix, angle, n_maps, cross, npix, None, C.byref(out)) == code
    assert _err(slicer._h) == "slicer_power_create: " + text
    assert not out.value


@pytest.mark.gpu
def test_kappa_add_refusals(slicer):
    kh = C.c_void_p()
    assert L.slicer_kappa_create(slicer._h, N, 1, C.byref(kh)) == 0
    try:
        maps = (C.c_void_p * 1)(None)
        coeff = np.ones(1)
        assert L.slicer_kappa_add(kh, 0, maps, coeff.ctypes.data) == ERR_ARG
        assert _err(slicer._h) == "slicer_kappa_add: n_maps = 0, expected 1..8"
        assert L.slicer_kappa_add(kh, 1, maps, coeff.ctypes.data) == ERR_ARG
        assert _err(slicer._h) == "slicer_kappa_add: map 0 is null"
    finally:
        L.slicer_kappa_destroy(kh)


@pytest.mark.gpu
def test_power_read_and_spectrum_state_refusals(slicer):
    ph = C.c_void_p()
    assert L.slicer_power_create(slicer._h, N, 5.0, 2, 0, N, None, C.byref(ph)) == 0
    d_map = slicer.to_device(np.zeros(N * N, np.float32))
    try:
        cl = np.zeros(2 * (N - 1))
        assert L.slicer_power_read(ph, cl.ctypes.data, None, None) == ERR_STATE
        assert _err(slicer._h) == "slicer_power_read before any slicer_power_run"
        maps = (C.c_void_p * 2)(d_map, d_map)
        assert L.slicer_power_run(ph, maps) == 0
        spec = np.zeros(N * (N // 2 + 1) * 2)
        assert L.slicer_power_spectrum(ph, 0, spec.ctypes.data) == ERR_STATE
        assert _err(slicer._h) == "slicer_power_spectrum: auto mode keeps only the last map's spectrum"
        assert L.slicer_power_spectrum(ph, 1, spec.ctypes.data) == 0
    finally:
        L.slicer_power_destroy(ph)
        slicer.free(d_map)
