"""Return codes and exact slicer_last_error texts of twelve add-on sub-handles (kappa, shear, power, moments, peaks,
rays, smooth, noise, minkowski, bispectrum, l1norm, betti): what their entry points answer without a handle, and -- on the
GPU -- before any run and for a map size outside the handle's.  The texts are not uniform (kappa, shear, power and bispectrum look at
the handle first, the others at the numbers) and are pinned as they are.  Messages of failed HIP calls carry a source
position and are not pinned here."""
import ctypes as C

import numpy as np
import pytest

import slicer_amd
from slicer_amd import lensing

L = lensing._L
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, 2, 3, 6
MAX = 131072  # the largest npix of the modules that have one, but Betti's
BETTI_MAX = 32768  # SLICER_BETTI_MAX_NPIX
EDGES = np.array([1.0, 3.0, 5.0])
E = EDGES.ctypes.data
BUF = np.zeros(64)
P = BUF.ctypes.data  # a pointer that is not null; nothing reads it before the handle has been refused


def _err(h=None):
    return (L.slicer_last_error(h) or b"").decode()


# ---- *_create without a handle -------------------------------------------------------------------
# name: (the arguments after npix of a well-formed call, numbers checked before the handle[, the largest npix])
CREATE = {
    "kappa": ((1,), False),
    "shear": ((5.0,), False),
    "power": ((5.0, 1, 0, 16, None), False),
    "moments": ((0, 0), True),
    "peaks": ((3, E), True),
    "rays": ((1.0,), True),
    "smooth": ((0, 2.0, 4.0), True),
    "noise": ((7,), True),
    "minkowski": ((3, E), True),
    "bispectrum": ((5.0, 3, E, 4, None), False),
    "l1norm": ((3, E), True),
    "betti": ((3, E), True, BETTI_MAX),
}


@pytest.mark.parametrize("null_out", [False, True])
@pytest.mark.parametrize("name", list(CREATE))
def test_create_without_a_handle(name, null_out):
    args, numbers_first, largest = (CREATE[name] + (MAX,))[:3]
    create = getattr(L, f"slicer_{name}_create")
    who = f"slicer_{name}_create: "
    expected = {0: (ERR_ARG, who + "npix must be positive"),
                largest + 1: (ERR_UNSUPPORTED, who + f"npix = {largest + 1} above {largest}"),
                16: (ERR_ARG, who + "null argument")}
    for npix in (0, largest + 1, 16):
        out = C.c_void_p(1)
        code, text = expected[npix if numbers_first else 16]
        assert create(None, npix, *args, None if null_out else C.byref(out)) == code, npix
        assert _err() == text
        # the numbers-first modules clear *out before anything else; the others return before they touch it
        assert out.value == (1 if null_out or not numbers_first else None)


# the four that take an ascending f64 table: (what its values are called, the refusal of too few, the most of them)
TABLES = {
    "peaks": ("edges", "fewer than 2 edges", 1025),
    "l1norm": ("edges", "fewer than 2 edges", 1025),
    "minkowski": ("thresholds", "fewer than 1 threshold", 1025),
    "betti": ("thresholds", "fewer than 1 threshold", 1025),
}


@pytest.mark.parametrize("name", list(TABLES))
def test_create_looks_at_the_table_before_the_handle(name):
    nouns, too_few, most = TABLES[name]
    create = getattr(L, f"slicer_{name}_create")
    who = f"slicer_{name}_create: "
    long, inf, nan, tie = (np.array(v, np.float64) for v in (np.arange(most + 1), [1, np.inf, 5], [1, np.nan, 5], [1, 3, 3]))
    cases = [((0, E), who + too_few), ((-1, E), who + too_few),
             ((most + 1, long.ctypes.data), who + f"{most + 1} {nouns}, at most {most}"),
             ((3, None), who + "null argument"),
             ((3, inf.ctypes.data), who + f"{nouns} must be finite"),
             ((3, nan.ctypes.data), who + f"{nouns} must be finite"),
             ((3, tie.ctypes.data), who + f"{nouns} must be strictly ascending"),
             ((most, long.ctypes.data), who + "null argument")]  # a table that is taken: now the handle is missed
    if too_few.startswith("fewer than 2"):
        cases.append(((1, E), who + too_few))
    for args, text in cases:
        out = C.c_void_p(1)
        assert create(None, 16, *args, C.byref(out)) == ERR_ARG, args
        assert _err() == text
        assert out.value is None


@pytest.mark.parametrize("name", list(CREATE))
def test_destroy_without_a_handle(name):
    L.slicer_power_read(None, None, None, None)  # leaves a text behind: destroy sets none
    assert getattr(L, f"slicer_{name}_destroy")(None) == ERR_ARG
    assert _err() == "slicer_power_read: null handle"


# ---- every other entry point without a handle ----------------------------------------------------
def _ref():
    return C.byref(C.c_void_p())


NULL_HANDLE = [
    ("slicer_kappa_add", (1, None, None), "slicer_kappa_add: null argument"),
    ("slicer_kappa_plane_means", (P, 1), "slicer_kappa_plane_means: null argument"),
    ("slicer_kappa_finalize", (), "null kappa handle"),
    ("slicer_kappa_reset", (), "null kappa handle"),
    ("slicer_kappa_device_map", (0, _ref()), "slicer_kappa_device_map: null argument"),
    ("slicer_kappa_read", (0, P), "slicer_kappa_device_map: null argument"),
    ("slicer_shear_run", (P,), "slicer_shear_run: null argument"),
    ("slicer_shear_spectrum", (P,), "slicer_shear_spectrum: null argument"),
    ("slicer_shear_device_map", (0, _ref()), "slicer_shear_device_map: null argument"),
    ("slicer_shear_read", (0, P), "slicer_shear_device_map: null argument"),
    ("slicer_shear_deflection", (), "slicer_shear_deflection: null argument"),
    ("slicer_shear_fd", (), "slicer_shear_fd: null argument"),
    ("slicer_power_run", (None,), "slicer_power_run: null argument"),
    ("slicer_power_spectrum", (0, P), "slicer_power_spectrum: null argument"),
    ("slicer_power_read", (P, None, None), "slicer_power_read: null handle"),
    ("slicer_moments_run", (P, None), "slicer_moments_run: null argument"),
    ("slicer_moments_read", (None, P, None, None), "slicer_moments_read: null handle"),
    ("slicer_moments_device_map", (1, _ref()), "slicer_moments_device_map: null argument"),
    ("slicer_moments_read_map", (1, P), "slicer_moments_read_map: null argument"),
    ("slicer_peaks_run", (P,), "slicer_peaks_run: null argument"),
    ("slicer_peaks_run_npix", (P, 16), "slicer_peaks_run_npix: null argument"),
    ("slicer_peaks_read", (P, None, None, None, None, None), "slicer_peaks_read: null handle"),
    ("slicer_rays_reset", (), "slicer_rays_reset: null handle"),
    ("slicer_rays_step", (1.0, None, P, P, P, P), "slicer_rays_step: null map"),
    ("slicer_rays_step", (1.0, P, P, P, P, P), "slicer_rays_step: null handle"),
    ("slicer_rays_observe", (1.0, None), "slicer_rays_observe: null argument"),
    ("slicer_rays_observe", (1.0, (C.c_void_p * 6)(P)), "slicer_rays_observe: null handle"),
    ("slicer_rays_state", (P,), "slicer_rays_state: null argument"),
    ("slicer_rays_planes", (None, None), "slicer_rays_planes: null handle"),
    ("slicer_smooth_run", (P,), "slicer_smooth_run: null argument"),
    ("slicer_smooth_run_npix", (P, 16), "slicer_smooth_run_npix: null argument"),
    ("slicer_smooth_device_map", (_ref(),), "slicer_smooth_device_map: null argument"),
    ("slicer_smooth_read", (P,), "slicer_smooth_read: null argument"),
    ("slicer_noise_run", (P, 1.0, 0, 0), "slicer_noise_run: null argument"),
    ("slicer_noise_run", (P, -1.0, 0, 0), "slicer_noise_run: sigma must be finite and not negative"),
    ("slicer_noise_run_npix", (P, 16, 1.0, 0, 0), "slicer_noise_run_npix: null argument"),
    ("slicer_noise_run_at", (P, 0, 16, 1.0, 0, 0), "slicer_noise_run_at: null argument"),
    ("slicer_noise_run_at", (P, 2, 16, 1.0, 0, 0),
     "slicer_noise_run_at: first_pixel must be a multiple of 4 (a run starts at a block)"),
    ("slicer_noise_words_device", (0, 1, 0, 0, P), "slicer_noise_words_device: null argument"),
    ("slicer_noise_device_map", (_ref(),), "slicer_noise_device_map: null argument"),
    ("slicer_noise_read", (P,), "slicer_noise_read: null argument"),
    ("slicer_minkowski_run", (P,), "slicer_minkowski_run: null argument"),
    ("slicer_minkowski_run_npix", (P, 16), "slicer_minkowski_run_npix: null argument"),
    ("slicer_minkowski_read", (P, None, None, None, None, None), "slicer_minkowski_read: null handle"),
    ("slicer_bispectrum_run", (P,), "slicer_bispectrum_run: null argument"),
    ("slicer_bispectrum_read", (P, None, None), "slicer_bispectrum_read: null handle"),
    ("slicer_bispectrum_spectrum", (P,), "slicer_bispectrum_spectrum: null argument"),
    ("slicer_bispectrum_read_map", (0, P), "slicer_bispectrum_read_map: null argument"),
    ("slicer_l1norm_run", (P,), "slicer_l1norm_run: null argument"),
    ("slicer_l1norm_run_npix", (P, 16), "slicer_l1norm_run_npix: null argument"),
    ("slicer_l1norm_read", (P, None, None, None, None, None, None), "slicer_l1norm_read: null handle"),
    ("slicer_betti_run", (P,), "slicer_betti_run: null argument"),
    ("slicer_betti_run_npix", (P, 16), "slicer_betti_run_npix: null argument"),
    ("slicer_betti_read", (P, None, None, None), "slicer_betti_read: null handle"),
]


@pytest.mark.parametrize("name,args,text", NULL_HANDLE, ids=[f"{c[0]}-{i}" for i, c in enumerate(NULL_HANDLE)])
def test_entry_points_without_a_handle(name, args, text):
    assert getattr(L, name)(None, *args) == ERR_ARG
    assert _err() == text


# ---- with a handle -------------------------------------------------------------------------------
N = 16


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@pytest.fixture(scope="module")
def d_zeros(slicer):
    d = slicer.to_device(np.zeros(N * N, np.float32))
    yield d
    slicer.free(d)


def _made(slicer, name, *args):
    out = C.c_void_p()
    assert getattr(L, f"slicer_{name}_create")(slicer._h, N, *args, C.byref(out)) == OK, _err(slicer._h)
    return out


def _state(slicer, code, text):
    assert code == ERR_STATE
    assert _err(slicer._h) == text


def _run_npix_refusals(slicer, name, handle, d_map, *more):
    run_npix = getattr(L, f"slicer_{name}_run_npix")
    for npix in (0, N + 1):
        assert run_npix(handle, d_map, npix, *more) == ERR_ARG
        assert _err(slicer._h) == f"slicer_{name}_run_npix: npix = {npix} outside 1..{N}"


@pytest.mark.gpu
def test_moments_before_any_run(slicer):
    mh = _made(slicer, "moments", 1, 0)
    try:
        _state(slicer, L.slicer_moments_read(mh, None, P, None, None), "slicer_moments_read before any slicer_moments_run")
        _state(slicer, L.slicer_moments_device_map(mh, 1, _ref()),
               "slicer_moments_device_map before any slicer_moments_run")
        _state(slicer, L.slicer_moments_read_map(mh, 1, P), "slicer_moments_device_map before any slicer_moments_run")
    finally:
        assert L.slicer_moments_destroy(mh) == OK


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["peaks", "minkowski", "l1norm", "betti"])
def test_counts_before_any_run_and_npix_outside(slicer, d_zeros, name):
    outputs = {"peaks": 6, "minkowski": 6, "l1norm": 7, "betti": 4}[name]  # arrays a *_read takes
    handle = _made(slicer, name, 3, E)
    try:
        _state(slicer, getattr(L, f"slicer_{name}_read")(handle, P, *[None] * (outputs - 1)),
               f"slicer_{name}_read before any slicer_{name}_run")
        for run, more in (("run", ()), ("run_npix", (N,))):  # a handle, but no map
            assert getattr(L, f"slicer_{name}_{run}")(handle, None, *more) == ERR_ARG
            assert _err(slicer._h) == f"slicer_{name}_{run}: null argument"
        _run_npix_refusals(slicer, name, handle, d_zeros)
    finally:
        assert getattr(L, f"slicer_{name}_destroy")(handle) == OK


@pytest.mark.gpu
def test_smooth_before_any_run_and_npix_outside(slicer, d_zeros):
    sh = _made(slicer, "smooth", 0, 1.0, 4.0)
    try:
        _state(slicer, L.slicer_smooth_read(sh, P), "slicer_smooth_read before any slicer_smooth_run")
        _state(slicer, L.slicer_smooth_device_map(sh, _ref()), "slicer_smooth_device_map before any slicer_smooth_run")
        _run_npix_refusals(slicer, "smooth", sh, d_zeros)
    finally:
        assert L.slicer_smooth_destroy(sh) == OK


@pytest.mark.gpu
def test_noise_before_any_run_and_npix_outside(slicer, d_zeros):
    nh = _made(slicer, "noise", 7)
    try:
        _state(slicer, L.slicer_noise_read(nh, P), "slicer_noise_read before any slicer_noise_run")
        _state(slicer, L.slicer_noise_device_map(nh, _ref()), "slicer_noise_device_map before any slicer_noise_run")
        _run_npix_refusals(slicer, "noise", nh, d_zeros, 1.0, 0, 0)
    finally:
        assert L.slicer_noise_destroy(nh) == OK


@pytest.mark.gpu
def test_bispectrum_before_any_run(slicer):
    bh = _made(slicer, "bispectrum", 5.0, 3, E, 4, None)
    try:
        _state(slicer, L.slicer_bispectrum_read(bh, P, None, None),
               "slicer_bispectrum_read of b or sums before any slicer_bispectrum_run")
        assert L.slicer_bispectrum_read(bh, None, P, None) == OK  # the triangle counts need no run
        _state(slicer, L.slicer_bispectrum_spectrum(bh, P), "slicer_bispectrum_spectrum before any slicer_bispectrum_run")
        _state(slicer, L.slicer_bispectrum_read_map(bh, 0, P), "slicer_bispectrum_read_map before any slicer_bispectrum_run")
    finally:
        assert L.slicer_bispectrum_destroy(bh) == OK
