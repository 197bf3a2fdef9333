"""Born-approximation convergence (kappa) maps from the lens planes, and the shear and lensing
potential maps from them (row N6), the binned auto and cross power spectra of such maps (row N7), the deflection
maps and finite-difference derivatives of the potential (row N8), and the central moments of such maps over a pyramid
of 2x2 halvings (row N9), and the one-point PDF histogram and peak / minimum counts of such maps (row N10), and
multi-plane ray tracing through the lens planes (row N11), and Gaussian and aperture-mass smoothing of such maps (row N12),
and shape noise for such maps from a counter-based generator (row N13), and the Minkowski functionals of such maps'
excursion sets as exact counts (row N14), and the binned bispectra of such maps (row N15), and the starlet transform of
such maps with the binned absolute sums of its scales, the starlet l1-norm (row N16), and the masked pseudo-C_l of such
maps: coupled bandpowers, the mask's mode-coupling matrix and the decoupled bandpowers (row N17), and the real-space
two-point correlation functions xi_kk, xi+ and xi- of such maps and of shear maps (row N18), and the Betti numbers of
such maps' excursion sets as exact counts (row N19), and the wavelet scattering coefficients of such maps (row N20), and
the E/B pseudo-C_l of masked shear maps: the spin-2 coupling matrices of the mask and the block decoupling (row N21), and
the catalogue of such maps' peaks and minima: positions, heights and sub-pixel offsets (row N22).

plane_weights wraps the host weights of include/slicer_amd.h (slicer_lensing_weights); Kappa is the device accumulator
(slicer_kappa_*) bound to a Slicer handle: it reads the finalized plane maps where they are, in HBM.  Shear (slicer_shear_*)
turns one kappa map into phi, gamma1, gamma2 and |gamma| on the same device, and on request into the deflection maps
(Shear.deflection) and the finite-difference alpha, kappa and shear of phi (Shear.fd; fd_derivatives for any device
map); Power (slicer_power_*) bins the spectra of several of them into C_l; Moments (slicer_moments_*) halves a map
level by level and sums the powers 2 ... 8 of every level's pixels about a centre; Peaks (slicer_peaks_*) counts a
map's pixels, peaks and minima by height over a list of edges; Rays (slicer_rays_*) shoots one ray per pixel through
the planes' deflection, convergence and shear maps (plane_strengths scales a mass plane to its lens map); Smooth
(slicer_smooth_*) filters a map with a truncated Gaussian or with the aperture-mass filter built from it; Noise
(slicer_noise_*) adds Gaussian noise that is a pure function of (seed, stream, realisation, pixel) to a map;
Minkowski (slicer_minkowski_*) counts the faces, edges and vertices of the pixel complex that lie in the sets x >= t_j;
Bispectrum (slicer_bispectrum_*) contracts the band-filtered f64 maps of a map over a list of bin triples; Starlet
(slicer_starlet_*) splits a map into wavelet scales that sum back to it, and L1Norm (slicer_l1norm_*) sums |x| of a map's
pixels bin by bin over Peaks' edges; Pcl (slicer_pcl_*) is Power under a mask (a border taper, a user mask or both),
with the coupling matrix of the mask and the bandpowers decoupled by it; Xi (slicer_xi_*) sums the pair products of
zero-padded maps over annuli of the lag, divided by the pair weights of one shared weight map; Betti (slicer_betti_*)
counts the 8-connected components of the sets x >= t_j and the holes in them by a union-find on the device; Scattering
(slicer_scattering_*) averages the moduli of a map's Morlet wavelet transforms, and of those moduli's transforms at
coarser scales; PclShear (slicer_pcl2_*) is Pcl for fields of (gamma1, gamma2) and optionally kappa: it rotates the
masked spectra to E and B, bins EE, EB, BB and the kappa crosses, and undoes the mask's mixing of E and B with the
spin-0, spin-2 and spin-4 coupling matrices; spin_phases gives the rotation's tables; PeakCatalogue
(slicer_catalogue_*) lists the peaks and minima that Peaks counts, in pixel order, and leaves the records on the device.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .api import Slicer, SlicerError

_L = _lib.load()


def _dptr(a):
    return a.ctypes.data if a is not None else None


def _host_chk(rc):
    """Raise the last error of a call that has no handle."""
    if rc:
        raise SlicerError(rc, (_L.slicer_last_error(None) or b"").decode())


class _SubHandle:
    """A handle made from a Slicer's: the attribute named by _handle holds it, the C call named by _destroy frees it."""
    _handle = _destroy = None

    def close(self):
        if getattr(self, self._handle, None):
            getattr(_L, self._destroy)(getattr(self, self._handle))
            setattr(self, self._handle, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _MapRuns:
    """run, run_kappa and run_level of a sub-handle whose runs take one f32 device map of at most its own npix: _run and
    _run_npix name the two C calls.  A class that keeps last_npix (the map size of the last run) has it recorded."""
    _run = _run_npix = None

    def run(self, d_map, npix=None):
        """d_map: device address of an f32 map of npix^2 pixels (None: the handle's npix; otherwise at most that)."""
        d = None if d_map is None else int(d_map)
        handle = getattr(self, self._handle)
        if npix is None:
            self._s._chk(getattr(_L, self._run)(handle, d))
        else:
            self._s._chk(getattr(_L, self._run_npix)(handle, d, int(npix)))
        if hasattr(self, "last_npix"):
            self.last_npix = self.npix if npix is None else int(npix)

    def run_kappa(self, kappa: "Kappa", s, **how):
        """The map of source s of a Kappa accumulator, where it is; `how`: what the class's run takes besides the map."""
        self.run(kappa.device_map(s), kappa.npix, **how)

    def run_level(self, moments: "Moments", level, **how):
        """Level `level` >= 1 of the last run of a Moments pyramid, where it is (level 0 is the caller's own map)."""
        self.run(moments.device_map(level), moments.npix >> int(level), **how)


def _plane_args(ld, ld2, zsnap, sources):
    """(ld, ld2, zsnap, zs, P, S) as slicer_lensing_* take them; zs is None for sources "all", and then S = P."""
    ld, ld2, zsnap = (np.ascontiguousarray(a, np.float64) for a in (ld, ld2, zsnap))
    P = ld.size
    assert ld2.size == P and zsnap.size == P
    zs = None if isinstance(sources, str) and sources == "all" else np.ascontiguousarray(sources, np.float64)
    return ld, ld2, zsnap, zs, P, P if zs is None else zs.size


def _read_outputs(slicer, npix, which, count, codes, run):
    """{code: f32 [npix, npix] array} for the codes 0 .. count-1 in `which`: their device buffers are allocated, filled
    by run(ptrs) (None where a code is not asked for), copied back and freed."""
    which = [int(w) for w in which]
    if any(not 0 <= w < count for w in which):
        raise ValueError(f"which: {codes} codes 0..{count - 1}")
    ptrs = [None] * count
    try:
        for w in set(which):
            ptrs[w] = slicer.malloc(4 * npix * npix)
        run(ptrs)
        return {w: slicer.to_host(ptrs[w], (npix, npix), np.float32) for w in which}
    finally:
        for p in ptrs:
            if p is not None:
                slicer.free(p)


def plane_weights(omega_m, omega_lambda, w0, fov_deg, npix, ld, ld2, zsnap, sources="all", growth=True, wa=0.0,
                  physical=False):
    """c[s, p] of kappa_s = sum_p c[s, p] (m_p - mean m_p), plus the per-plane zlo, zup, zl, chil and the source list.

    ld, ld2: comoving plane edges in Mpc/h (Lens.ld / ld2); zsnap: snapshot redshift of every plane (Lens.zfromsnap);
    sources: "all" (the far-edge redshift of every plane) or a sequence of source redshifts."""
    ld, ld2, zsnap, zs, P, S = _plane_args(ld, ld2, zsnap, sources)
    coeff = np.zeros((S, P), np.float64)
    out = {k: np.zeros(P, np.float64) for k in ("zlo", "zup", "zl", "chil")}
    _host_chk(_L.slicer_lensing_weights(float(omega_m), float(omega_lambda), float(w0), float(wa), float(fov_deg),
                                        int(npix), int(bool(growth)), int(bool(physical)), P, _dptr(ld), _dptr(ld2),
                                        _dptr(zsnap), S, _dptr(zs), _dptr(coeff), _dptr(out["zlo"]), _dptr(out["zup"]),
                                        _dptr(out["zl"]), _dptr(out["chil"])))
    out["c"] = coeff
    out["zs"] = out["zup"].copy() if zs is None else zs
    return out


def plane_strengths(omega_m, omega_lambda, w0, fov_deg, npix, ld, ld2, zsnap, sources="all", growth=True, wa=0.0,
                    physical=False):
    """The per-plane lensing strengths of the ray tracer (slicer_lensing_plane_strengths), arguments as plane_weights:
    dict with strength [P] (the lens map of plane p is strength[p] (m_p - mean m_p)), chil [P], zs, chis [S] and
    n_in_front [S] (the planes in front of every source)."""
    ld, ld2, zsnap, zs, P, S = _plane_args(ld, ld2, zsnap, sources)
    out = {"strength": np.zeros(P, np.float64), "chil": np.zeros(P, np.float64), "chis": np.zeros(S, np.float64),
           "n_in_front": np.zeros(S, np.int32)}
    _host_chk(_L.slicer_lensing_plane_strengths(float(omega_m), float(omega_lambda), float(w0), float(wa),
                                                float(fov_deg), int(npix), int(bool(growth)), int(bool(physical)), P,
                                                _dptr(ld), _dptr(ld2), _dptr(zsnap), S, _dptr(zs),
                                                _dptr(out["strength"]), _dptr(out["chil"]), _dptr(out["chis"]),
                                                _dptr(out["n_in_front"])))
    if zs is None:
        zs = plane_weights(omega_m, omega_lambda, w0, fov_deg, npix, ld, ld2, zsnap, "all", growth, wa, physical)["zs"]
    out["zs"] = zs
    return out


class Kappa(_SubHandle):
    """n_sources kappa maps of npix^2 pixels accumulated on the device of `slicer`, on its stream."""
    _handle, _destroy = "_kh", "slicer_kappa_destroy"

    def __init__(self, slicer: Slicer, npix, n_sources):
        self._s = slicer
        self.npix, self.n_sources = int(npix), int(n_sources)
        self.n_added = 0
        self._dirty = True
        kh = C.c_void_p()
        slicer._chk(_L.slicer_kappa_create(slicer._h, self.npix, self.n_sources, C.byref(kh)))
        self._kh = kh

    def add_device(self, ptrs, coeff):
        """ptrs: device addresses of n_maps f32 maps; coeff: [n_maps][n_sources] weights."""
        ptrs = [int(p) for p in ptrs]
        coeff = np.ascontiguousarray(coeff, np.float64).reshape(len(ptrs), self.n_sources)
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._s._chk(_L.slicer_kappa_add(self._kh, len(ptrs), arr, coeff.ctypes.data))
        self.n_added += len(ptrs)
        self._dirty = True

    def add(self, plane_indices, coeff):
        """The total maps of planes `plane_indices` of the slicer's current (finalized) pass."""
        self.add_device([self._s.plane_device_maps(int(i))[0] for i in plane_indices], coeff)

    def finalize(self):
        self._s._chk(_L.slicer_kappa_finalize(self._kh))
        self._dirty = False

    def reset(self):
        """Zero the accumulators and forget the means: the handle as just created."""
        self._s._chk(_L.slicer_kappa_reset(self._kh))
        self.n_added = 0
        self._dirty = True

    def plane_means(self):
        out = np.zeros(self.n_added, np.float64)
        self._s._chk(_L.slicer_kappa_plane_means(self._kh, out.ctypes.data, self.n_added))
        return out

    def device_map(self, s):
        if self._dirty:
            self.finalize()
        p = C.c_void_p()
        self._s._chk(_L.slicer_kappa_device_map(self._kh, int(s), C.byref(p)))
        return p.value

    def read(self, s):
        if self._dirty:
            self.finalize()
        out = np.empty((self.npix, self.npix), np.float32)
        self._s._chk(_L.slicer_kappa_read(self._kh, int(s), out.ctypes.data))
        return out


SHEAR_PHI, SHEAR_GAMMA1, SHEAR_GAMMA2, SHEAR_GAMMA = 0, 1, 2, 3
SHEAR_ALPHA1, SHEAR_ALPHA2 = 8, 9
FD_ALPHA1, FD_ALPHA2, FD_KAPPA, FD_GAMMA1, FD_GAMMA2, FD_GAMMA = range(6)
FD_COUNT = 6
SHEAR_FD_ALPHA1, SHEAR_FD_ALPHA2, SHEAR_FD_KAPPA, SHEAR_FD_GAMMA1, SHEAR_FD_GAMMA2, SHEAR_FD_GAMMA = range(16, 22)


def shear_supported(npix):
    """True if Shear takes npix (2 ... 16384, prime factors 2, 3, 5, 7 only); host only, no device needed."""
    return bool(_L.slicer_shear_supported(int(npix)))


class Shear(_SubHandle):
    """Lensing potential phi and shear gamma1, gamma2, |gamma| of npix^2 kappa maps of side angle_deg degrees,
    computed on the device of `slicer`, on its stream.  read / device_map take SHEAR_*."""
    _handle, _destroy = "_sh", "slicer_shear_destroy"

    def __init__(self, slicer: Slicer, npix, angle_deg):
        self._s = slicer
        self.npix, self.angle_deg = int(npix), float(angle_deg)
        sh = C.c_void_p()
        slicer._chk(_L.slicer_shear_create(slicer._h, self.npix, self.angle_deg, C.byref(sh)))
        self._sh = sh
        self.last_input = None  # the device address handed to the last run

    def run(self, d_kappa):
        """d_kappa: device address of an f32 npix^2 map."""
        self._s._chk(_L.slicer_shear_run(self._sh, int(d_kappa)))
        self.last_input = int(d_kappa)

    def run_kappa(self, kappa: Kappa, s):
        """The map of source s of a Kappa accumulator, where it is."""
        self.run(kappa.device_map(s))

    def spectrum(self):
        """rfft2 of the last run's input, [npix, npix // 2 + 1] complex128."""
        out = np.empty((self.npix, self.npix // 2 + 1), np.complex128)
        self._s._chk(_L.slicer_shear_spectrum(self._sh, out.ctypes.data))
        return out

    def deflection(self):
        """The deflection maps of the last run (read / device_map with SHEAR_ALPHA1, SHEAR_ALPHA2)."""
        self._s._chk(_L.slicer_shear_deflection(self._sh))

    def fd(self):
        """The finite-difference maps of the last run's phi (read / device_map with SHEAR_FD_*)."""
        self._s._chk(_L.slicer_shear_fd(self._sh))

    def device_map(self, which):
        p = C.c_void_p()
        self._s._chk(_L.slicer_shear_device_map(self._sh, int(which), C.byref(p)))
        return p.value

    def read(self, which):
        out = np.empty((self.npix, self.npix), np.float32)
        self._s._chk(_L.slicer_shear_read(self._sh, int(which), out.ctypes.data))
        return out


def fd_run(slicer: Slicer, d_phi, npix, spacing, ptrs):
    """slicer_fd_derivatives as it is: ptrs are FD_COUNT device addresses of npix^2 f32 buffers, None to skip one."""
    arr = (C.c_void_p * FD_COUNT)(*[None if p is None else int(p) for p in ptrs])
    slicer._chk(_L.slicer_fd_derivatives(slicer._h, int(npix), float(spacing), None if d_phi is None else int(d_phi), arr))


def fd_derivatives(slicer: Slicer, d_phi, npix, spacing, which=tuple(range(FD_COUNT))):
    """Finite-difference derivatives of the f32 npix^2 device map at address d_phi, samples
    `spacing` apart: {code: f32 [npix, npix] array} for the FD_* codes in `which`."""
    return _read_outputs(slicer, int(npix), which, FD_COUNT, "FD_*",
                         lambda ptrs: fd_run(slicer, d_phi, npix, spacing, ptrs))


def ell_fundamental(angle_deg):
    """l_f = 2 pi / theta of a map of side angle_deg degrees, rounded as slicer_power_* round it."""
    return 2.0 * math.pi / (float(angle_deg) * math.pi / 180.0)


def _edges(npix, edges, ell_edges, angle_deg):
    """(n_edges, f64 array or None) of edges in units of l_f; ell_edges are divided by l_f on the host."""
    if edges is not None and ell_edges is not None:
        raise ValueError("give edges or ell_edges, not both")
    if ell_edges is not None:
        if not (math.isfinite(angle_deg) and angle_deg > 0):
            raise ValueError("ell_edges need a positive, finite angle")
        edges = np.asarray(ell_edges, np.float64) / ell_fundamental(angle_deg)
    if edges is None:
        return int(npix), None
    edges = np.ascontiguousarray(edges, np.float64).ravel()
    return edges.size, edges


def power_bins(npix, edges=None):
    """Host only (no device): {"counts": N_b int64, "mean_radius": mean sqrt(m2) per bin in units of l_f} for the
    edges (units of l_f; None: 0, 1, ..., npix - 1)."""
    n_edges, e = _edges(npix, edges, None, 1.0)
    B = max(n_edges - 1, 0)
    counts = np.zeros(B, np.int64)
    mean = np.zeros(B, np.float64)
    _host_chk(_L.slicer_power_bins(int(npix), n_edges, _dptr(e), counts.ctypes.data, mean.ctypes.data))
    return {"counts": counts, "mean_radius": mean}


class Power(_SubHandle):
    """Binned power spectra C_l of n_maps npix^2 maps of side angle_deg degrees, on the device of `slicer`, on its
    stream.  cross=False: the auto-spectra; cross=True: every pair.  edges in units of
    l_f = 2 pi / theta (None: 0, 1, ..., npix - 1), or ell_edges in multipoles."""
    _handle, _destroy = "_ph", "slicer_power_destroy"

    def __init__(self, slicer: Slicer, npix, angle_deg, n_maps, cross=False, edges=None, ell_edges=None):
        self._s = slicer
        self.npix, self.angle_deg, self.n_maps, self.cross = int(npix), float(angle_deg), int(n_maps), bool(cross)
        ok = math.isfinite(self.angle_deg) and self.angle_deg > 0  # otherwise slicer_power_create refuses it
        self.ell_f = ell_fundamental(self.angle_deg) if ok else math.nan
        n_edges, e = _edges(self.npix, edges, ell_edges, self.angle_deg)
        self.edges = np.arange(self.npix, dtype=np.float64) if e is None else e.copy()
        self.n_bins = n_edges - 1
        ph = C.c_void_p()
        slicer._chk(_L.slicer_power_create(slicer._h, self.npix, self.angle_deg, self.n_maps, int(self.cross), n_edges,
                                           _dptr(e), C.byref(ph)))
        self._ph = ph

    def run(self, ptrs):
        """ptrs: device addresses of the n_maps f32 npix^2 maps."""
        ptrs = [int(p) for p in ptrs]
        if len(ptrs) != self.n_maps:
            raise ValueError(f"expected {self.n_maps} maps, got {len(ptrs)}")
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._s._chk(_L.slicer_power_run(self._ph, arr))

    def run_kappa(self, kappa: Kappa):
        """The maps of every source of a Kappa accumulator, where they are."""
        self.run([kappa.device_map(s) for s in range(kappa.n_sources)])

    def spectrum(self, map):
        """rfft2 of map `map` of the last run, [npix, npix // 2 + 1] complex128 (auto mode: the last map only)."""
        out = np.empty((self.npix, self.npix // 2 + 1), np.complex128)
        self._s._chk(_L.slicer_power_spectrum(self._ph, int(map), out.ctypes.data))
        return out

    def read(self):
        """dict: ell_lo, ell_hi (bin edges in multipoles), ell (mean l), counts, and cl: [S][S][B], symmetric (cross)
        or [S][B] (auto)."""
        S, B = self.n_maps, self.n_bins
        npairs = S * (S + 1) // 2 if self.cross else S
        flat = np.empty((npairs, B), np.float64)
        ell = np.empty(B, np.float64)
        counts = np.empty(B, np.int64)
        self._s._chk(_L.slicer_power_read(self._ph, flat.ctypes.data, ell.ctypes.data, counts.ctypes.data))
        if self.cross:
            cl = np.empty((S, S, B), np.float64)
            p = 0
            for s in range(S):
                for t in range(s, S):
                    cl[s, t] = cl[t, s] = flat[p]
                    p += 1
        else:
            cl = flat
        return {"ell_lo": self.edges[:-1] * self.ell_f, "ell_hi": self.edges[1:] * self.ell_f, "ell": ell,
                "counts": counts, "cl": cl}


HALVE_MEAN, HALVE_SUM = 0, 1
MOMENTS_ORDERS = 7  # k = 2 ... 8


def moments_depth(npix):
    """D(npix): the f64 additions on the longest path of the summation trees of an npix^2 level (the D of the bounds
    in include/slicer_amd.h); host only, no device needed."""
    d = _L.slicer_moments_depth(int(npix))
    _host_chk(2 if d < 0 else 0)
    return d


class Moments(_SubHandle):
    """Central moments of orders 2 ... 8 of an npix^2 map and of `levels` successive 2x2 halvings of it, on the device
    of `slicer`, on its stream.  mode "mean" halves to block means (kappa), "sum" to block sums
    (mass planes, Lens/halve.py)."""
    _handle, _destroy = "_mh", "slicer_moments_destroy"

    def __init__(self, slicer: Slicer, npix, levels=0, mode="mean"):
        if mode not in ("mean", "sum"):
            raise ValueError('mode: "mean" or "sum"')
        self._s = slicer
        self.npix, self.levels, self.mode = int(npix), int(levels), mode
        mh = C.c_void_p()
        slicer._chk(_L.slicer_moments_create(slicer._h, self.npix, self.levels, HALVE_SUM if mode == "sum" else HALVE_MEAN,
                                             C.byref(mh)))
        self._mh = mh

    def run(self, d_map, centres=None):
        """d_map: device address of an f32 npix^2 map; centres: None (every level's own mean) or levels + 1 values,
        NaN where a level is to take its own mean."""
        c = None
        if centres is not None:
            c = np.ascontiguousarray(centres, np.float64).ravel()
            if c.size != self.levels + 1:
                raise ValueError(f"expected {self.levels + 1} centres, got {c.size}")
        self._s._chk(_L.slicer_moments_run(self._mh, int(d_map), _dptr(c)))

    def run_kappa(self, kappa: Kappa, s, centres=None):
        """The map of source s of a Kappa accumulator, where it is."""
        self.run(kappa.device_map(s), centres)

    def read(self):
        """dict: npix [levels+1], mean, centre (the ones used), sums [levels+1, 7] = S_2 ... S_8, moments = sums / npix^2."""
        n = self.levels + 1
        npix = np.empty(n, np.int32)
        mean, centre = np.empty(n, np.float64), np.empty(n, np.float64)
        sums = np.empty((n, MOMENTS_ORDERS), np.float64)
        self._s._chk(_L.slicer_moments_read(self._mh, npix.ctypes.data, mean.ctypes.data, centre.ctypes.data,
                                            sums.ctypes.data))
        return {"npix": npix, "mean": mean, "centre": centre, "sums": sums,
                "moments": sums / (npix.astype(np.float64) ** 2)[:, None]}

    def device_map(self, level):
        p = C.c_void_p()
        self._s._chk(_L.slicer_moments_device_map(self._mh, int(level), C.byref(p)))
        return p.value

    def read_map(self, level):
        n = self.npix >> int(level) if 0 <= int(level) <= self.levels else 1
        out = np.empty((n, n), np.float32)
        self._s._chk(_L.slicer_moments_read_map(self._mh, int(level), out.ctypes.data))
        return out


def combine_moments(reads):
    """m_k of several realisations as Lens/moment.py averages them: sum_f S_k(f) / (F N), [levels+1, 7], from the
    Moments.read() of every realisation (all run about the same centres)."""
    reads = list(reads)
    if not reads:
        raise ValueError("no reads to combine")
    npix = reads[0]["npix"]
    total = np.zeros_like(reads[0]["sums"])
    for r in reads:
        if not np.array_equal(r["npix"], npix):
            raise ValueError("the reads are of different pyramids")
        total = total + r["sums"]
    return total / len(reads) / (npix.astype(np.float64) ** 2)[:, None]


PEAKS_MAX_BINS = 1024


def peaks_edges(lo, hi, bins):
    """bins + 1 uniform f64 edges as slicer_peaks_edges rounds them: e_0 = lo, e_B = hi, e_b = lo + b * ((hi - lo) / B)
    between; host only, no device needed."""
    bins = int(bins)
    e = np.zeros(max(bins, 0) + 1, np.float64)
    _host_chk(_L.slicer_peaks_edges(float(lo), float(hi), bins, e.ctypes.data))
    return e


class Peaks(_MapRuns, _SubHandle):
    """One-point PDF histogram and the counts of peaks and minima by height of an npix^2 map over the f64 `edges`, on
    the device of `slicer`, on its stream.  Every count is an exact int64."""
    _handle, _destroy = "_ph", "slicer_peaks_destroy"
    _run, _run_npix = "slicer_peaks_run", "slicer_peaks_run_npix"

    def __init__(self, slicer: Slicer, npix, edges):
        self._s = slicer
        self.npix = int(npix)
        self.edges = np.array(edges, np.float64).ravel()
        self.n_bins = self.edges.size - 1
        ph = C.c_void_p()
        slicer._chk(_L.slicer_peaks_create(slicer._h, self.npix, self.edges.size, _dptr(self.edges), C.byref(ph)))
        self._ph = ph

    def read(self):
        """dict: edges [B+1], pdf, peaks, minima (int64 [B]), below, above (int64 [3]: pdf, peaks, minima), nan."""
        B = self.n_bins
        pdf, peaks, minima = (np.empty(B, np.int64) for _ in range(3))
        below, above, nan = np.empty(3, np.int64), np.empty(3, np.int64), np.empty(1, np.int64)
        self._s._chk(_L.slicer_peaks_read(self._ph, pdf.ctypes.data, peaks.ctypes.data, minima.ctypes.data,
                                          below.ctypes.data, above.ctypes.data, nan.ctypes.data))
        return {"edges": self.edges.copy(), "pdf": pdf, "peaks": peaks, "minima": minima, "below": below, "above": above,
                "nan": int(nan[0])}


MINKOWSKI_MAX_THRESHOLDS = 1025


class Minkowski(_MapRuns, _SubHandle):
    """The Minkowski functionals of the excursion sets x >= t_j of an npix^2 map over the f64 `thresholds`, as exact
    int64 counts of the faces, edges and vertices of the pixel complex, on the device of `slicer`, on its stream
    (DESIGN.md S8 row N14).  peaks_edges(lo, hi, bins) gives bins + 1 uniform thresholds."""
    _handle, _destroy = "_mh", "slicer_minkowski_destroy"
    _run, _run_npix = "slicer_minkowski_run", "slicer_minkowski_run_npix"

    def __init__(self, slicer: Slicer, npix, thresholds):
        self._s = slicer
        self.npix = int(npix)
        self.thresholds = np.array(thresholds, np.float64).ravel()
        self.n_thresholds = self.thresholds.size
        mh = C.c_void_p()
        slicer._chk(_L.slicer_minkowski_create(slicer._h, self.npix, self.n_thresholds, _dptr(self.thresholds),
                                               C.byref(mh)))
        self._mh = mh
        self.last_npix = None  # of the last run

    def read(self):
        """dict: thresholds [T], faces, edges, vertices, boundary, border and euler = vertices - edges + faces (int64
        [T], one value per threshold), nan, and npix: the map size of the last run."""
        T = self.n_thresholds
        faces, edges, vertices, boundary, border = (np.empty(T, np.int64) for _ in range(5))
        nan = np.empty(1, np.int64)
        self._s._chk(_L.slicer_minkowski_read(self._mh, faces.ctypes.data, edges.ctypes.data, vertices.ctypes.data,
                                              boundary.ctypes.data, border.ctypes.data, nan.ctypes.data))
        return {"thresholds": self.thresholds.copy(), "faces": faces, "edges": edges, "vertices": vertices,
                "boundary": boundary, "border": border, "euler": vertices - edges + faces, "nan": int(nan[0]),
                "npix": self.last_npix}


def minkowski_functionals(read, angle_deg):
    """The counts of a Minkowski.read() of a map of angle_deg degrees a side as densities; host only.  With npix =
    read["npix"], theta = angle_deg * pi / 180 and the pixel side d = theta / npix, each one f64 expression:
      v0 = faces / npix^2                              the area fraction
      v1 = boundary * d / (4 * theta^2)                a quarter of the outline's length inside the field per area
      v1_with_border = (boundary + border) * d / (4 * theta^2)   the same with the part on the map's rim
      v2 = euler / theta^2                             the Euler characteristic per area
    v1 is the Manhattan length of a pixelised outline: for an isotropic smooth field it overestimates the length of the
    smooth contour by about 4 / pi.  That is reported as it is, not corrected."""
    npix = int(read["npix"])
    theta = float(angle_deg) * math.pi / 180.0
    d = theta / npix
    f64 = lambda k: np.asarray(read[k], np.int64).astype(np.float64)
    return {"thresholds": np.array(read["thresholds"], np.float64),
            "v0": f64("faces") / (float(npix) * float(npix)),
            "v1": f64("boundary") * d / (4.0 * theta * theta),
            "v1_with_border": (f64("boundary") + f64("border")) * d / (4.0 * theta * theta),
            "v2": f64("euler") / (theta * theta)}


BETTI_MAX_THRESHOLDS = 1025
BETTI_MAX_NPIX = 32768


class Betti(_MapRuns, _SubHandle):
    """The Betti numbers of the excursion sets x >= t_j of an npix^2 map over the f64 `thresholds`, as exact int64
    counts: the 8-connected components of every set and its holes (the 4-connected components of the complement that
    do not touch the map's rim), on the device of `slicer`, on its stream.  components - holes
    is Minkowski's euler of the same map and thresholds.  peaks_edges(lo, hi, bins) gives bins + 1 uniform thresholds."""
    _handle, _destroy = "_bh", "slicer_betti_destroy"
    _run, _run_npix = "slicer_betti_run", "slicer_betti_run_npix"

    def __init__(self, slicer: Slicer, npix, thresholds):
        self._s = slicer
        self.npix = int(npix)
        self.thresholds = np.array(thresholds, np.float64).ravel()
        self.n_thresholds = self.thresholds.size
        bh = C.c_void_p()
        slicer._chk(_L.slicer_betti_create(slicer._h, self.npix, self.n_thresholds, _dptr(self.thresholds),
                                           C.byref(bh)))
        self._bh = bh
        self.last_npix = None  # of the last run

    def read(self):
        """dict: thresholds [T], components, holes, faces (int64 [T], one value per threshold), nan, and npix: the map
        size of the last run."""
        T = self.n_thresholds
        components, holes, faces = (np.empty(T, np.int64) for _ in range(3))
        nan = np.empty(1, np.int64)
        self._s._chk(_L.slicer_betti_read(self._bh, components.ctypes.data, holes.ctypes.data, faces.ctypes.data,
                                          nan.ctypes.data))
        return {"thresholds": self.thresholds.copy(), "components": components, "holes": holes, "faces": faces,
                "nan": int(nan[0]), "npix": self.last_npix}


CATALOGUE_MAX_NPIX = 32768
CATALOGUE_MAX_CAPACITY = 1 << 29
CATALOGUE_PEAKS, CATALOGUE_MINIMA = 1, 2    # kinds
CATALOGUE_MINIMUM, CATALOGUE_FALLBACK = 1, 2  # flags
# slicer_catalogue_record (_lib.CatalogueRecord): 32 bytes
CATALOGUE_DTYPE = np.dtype([("row", "<i4"), ("col", "<i4"), ("value", "<f4"), ("flags", "<u4"), ("dy", "<f8"), ("dx", "<f8")])


class PeakCatalogue(_MapRuns, _SubHandle):
    """The peaks and minima of an npix^2 map -- those that Peaks counts -- as records (row, col, value, flags, dy, dx) in
    ascending row * npix + col, with the sub-pixel offset (dy, dx) of a quadratic fit to the 3 x 3 window, on the device
    of `slicer`, on its stream.  The handle holds `capacity` records; a run counts every kept
    peak and minimum and stores the first `capacity` of them.  d_records: the address of a device buffer of the caller's
    for the records (32 * capacity bytes, on the 16-byte grid) instead of one of the handle's own."""
    _handle, _destroy = "_ch", "slicer_catalogue_destroy"

    def __init__(self, slicer: Slicer, npix, capacity, d_records=None):
        self._s = slicer
        self.npix = int(npix)
        self.capacity = int(capacity)
        ch = C.c_void_p()
        slicer._chk(_L.slicer_catalogue_create(slicer._h, self.npix, self.capacity,
                                               None if d_records is None else int(d_records), C.byref(ch)))
        self._ch = ch
        self.last_npix = None  # of the last run

    def run(self, d_map, npix=None, kinds=CATALOGUE_PEAKS, min_peak=-math.inf, max_minimum=math.inf):
        """d_map: device address of an f32 map of npix^2 pixels (None: the handle's npix; otherwise at most that).
        kinds: CATALOGUE_PEAKS | CATALOGUE_MINIMA; a peak is kept iff its value >= min_peak, a minimum iff <= max_minimum."""
        d = None if d_map is None else int(d_map)
        self._s._chk(_L.slicer_catalogue_run_npix(self._ch, d, int(kinds), float(min_peak), float(max_minimum),
                                                  self.npix if npix is None else int(npix)))
        self.last_npix = self.npix if npix is None else int(npix)

    def counts(self):
        """dict: peaks, minima (the kept ones of the last run, whatever the capacity), stored, and npix of that run."""
        n = [C.c_int64() for _ in range(3)]
        self._s._chk(_L.slicer_catalogue_count(self._ch, *(C.byref(v) for v in n)))
        return {"peaks": n[0].value, "minima": n[1].value, "stored": n[2].value, "npix": self.last_npix}

    def read(self, max_records=None):
        """The stored records of the last run (at most max_records of them), a structured array of CATALOGUE_DTYPE."""
        most = self.capacity if max_records is None else int(max_records)
        stored = C.c_int64()
        self._s._chk(_L.slicer_catalogue_count(self._ch, None, None, C.byref(stored)))
        out = np.empty(max(0, min(most, stored.value)), CATALOGUE_DTYPE)
        copied = C.c_int64()
        self._s._chk(_L.slicer_catalogue_read(self._ch, out.ctypes.data if out.size else None, out.size, C.byref(copied)))
        return out[:copied.value]

    def device_records(self):
        """(address of the records, address of the int64 {peaks, minima, stored}) of the last run, on the device: valid
        until the next run or close."""
        r, c = C.c_void_p(), C.c_void_p()
        self._s._chk(_L.slicer_catalogue_device(self._ch, C.byref(r), C.byref(c)))
        return r.value, c.value


BISPECTRUM_MAX_BINS = 32


def bispectrum_triples(n_bins, kind="all"):
    """The triples i <= j <= k of n_bins bins, int32 [n, 3]: "all" B (B + 1) (B + 2) / 6 of them in lexicographic order,
    or the "equilateral" ones (b, b, b)."""
    B = int(n_bins)
    if kind == "equilateral":
        t = [(b, b, b) for b in range(B)]
    elif kind == "all":
        t = [(i, j, k) for i in range(B) for j in range(i, B) for k in range(j, B)]
    else:
        raise ValueError('kind: "all" or "equilateral"')
    return np.array(t, np.int32).reshape(-1, 3)


def _triples(n_bins, triples):
    """int32 [n, 3] from "all", "equilateral", None (all) or an array of rows (i, j, k)."""
    if triples is None or isinstance(triples, str):
        return bispectrum_triples(n_bins, "all" if triples is None else triples)
    t = np.ascontiguousarray(triples, np.int32)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("triples: rows (i, j, k)")
    return t


def bispectrum_triangles(npix, edges=None, triples=None):
    """Host only (no device): the exact number of closed triangles T_ijk (int64) of every triple (None: all of them) for
    the edges (units of l_f; None: 0, 1, ..., npix - 1), by enumeration (slicer_bispectrum_triangles)."""
    n_edges, e = _edges(npix, edges, None, 1.0)
    t = _triples(max(n_edges - 1, 0), triples)
    out = np.zeros(t.shape[0], np.int64)
    _host_chk(_L.slicer_bispectrum_triangles(int(npix), n_edges, _dptr(e), t.shape[0], _dptr(t), out.ctypes.data))
    return out


class Bispectrum(_SubHandle):
    """Binned bispectra B_ijk of an npix^2 map of side angle_deg degrees over a list of bin triples, on the device of
    `slicer`, on its stream.  edges in units of l_f = 2 pi / theta, or ell_edges in multipoles,
    at most 32 bins; triples "all", "equilateral" or rows (i, j, k) with i <= j <= k."""
    _handle, _destroy = "_bh", "slicer_bispectrum_destroy"

    def __init__(self, slicer: Slicer, npix, angle_deg, edges=None, ell_edges=None, triples="all"):
        self._s = slicer
        self.npix, self.angle_deg = int(npix), float(angle_deg)
        ok = math.isfinite(self.angle_deg) and self.angle_deg > 0  # otherwise slicer_bispectrum_create refuses it
        self.ell_f = ell_fundamental(self.angle_deg) if ok else math.nan
        n_edges, e = _edges(self.npix, edges, ell_edges, self.angle_deg)
        self.edges = np.arange(self.npix, dtype=np.float64) if e is None else e.copy()
        self.n_bins = n_edges - 1
        # (more than 32 bins: "all" would be a long list that the create call refuses anyway, so it gets one triple)
        many = self.n_bins > BISPECTRUM_MAX_BINS and (triples is None or isinstance(triples, str))
        self.triples = np.zeros((1, 3), np.int32) if many else _triples(self.n_bins, triples)
        bh = C.c_void_p()
        slicer._chk(_L.slicer_bispectrum_create(slicer._h, self.npix, self.angle_deg, n_edges, _dptr(e),
                                                self.triples.shape[0], _dptr(self.triples), C.byref(bh)))
        self._bh = bh

    def run(self, d_map):
        """d_map: device address of an f32 npix^2 map."""
        self._s._chk(_L.slicer_bispectrum_run(self._bh, None if d_map is None else int(d_map)))

    def run_kappa(self, kappa: Kappa, s):
        """The map of source s of a Kappa accumulator, where it is."""
        self.run(kappa.device_map(s))

    def triangles(self):
        """T_ijk as the device summed them at create (f64, not rounded); readable before any run."""
        t = np.empty(self.triples.shape[0], np.float64)
        self._s._chk(_L.slicer_bispectrum_read(self._bh, None, t.ctypes.data, None))
        return t

    def read(self):
        """dict: b (B_ijk, NaN for a triple without a closed triangle), triangles (T_ijk), sums (the raw S_ijk), triples
        [n, 3], and per bin ell_mean and counts (the half-plane modes, m2 = 0 included) from power_bins."""
        n = self.triples.shape[0]
        b, t, s = (np.empty(n, np.float64) for _ in range(3))
        self._s._chk(_L.slicer_bispectrum_read(self._bh, b.ctypes.data, t.ctypes.data, s.ctypes.data))
        bins = power_bins(self.npix, self.edges)
        return {"b": b, "triangles": t, "sums": s, "triples": self.triples.copy(),
                "ell_mean": bins["mean_radius"] * self.ell_f, "counts": bins["counts"]}

    def spectrum(self):
        """rfft2 of the last run's input, [npix, npix // 2 + 1] complex128."""
        out = np.empty((self.npix, self.npix // 2 + 1), np.complex128)
        self._s._chk(_L.slicer_bispectrum_spectrum(self._bh, out.ctypes.data))
        return out

    def read_map(self, bin):
        """F_bin of the last run, f64 [npix, npix]."""
        out = np.empty((self.npix, self.npix), np.float64)
        self._s._chk(_L.slicer_bispectrum_read_map(self._bh, int(bin), out.ctypes.data))
        return out


SMOOTH_GAUSS, SMOOTH_MAP = 0, 1
SMOOTH_MAX_RADIUS = 128
_SMOOTH_KINDS = {"gauss": SMOOTH_GAUSS, "map": SMOOTH_MAP}


def smooth_weights(sigma_pix, truncate=4.0):
    """(R, g, h) as slicer_smooth_weights makes them: the radius floor(truncate sigma_pix + 0.5) and the f64 tables
    g_k = exp(-q_k), h_k = q_k g_k, q_k = k^2 / (2 sigma_pix^2), k = 0 ... R; host only, no device needed."""
    R = C.c_int32()
    _host_chk(_L.slicer_smooth_weights(float(sigma_pix), float(truncate), C.byref(R), None, None))
    g, h = np.empty(R.value + 1, np.float64), np.empty(R.value + 1, np.float64)
    _host_chk(_L.slicer_smooth_weights(float(sigma_pix), float(truncate), None, g.ctypes.data, h.ctypes.data))
    return R.value, g, h


class Smooth(_MapRuns, _SubHandle):
    """An npix^2 map filtered with a Gaussian of sigma_pix pixels truncated at `truncate` sigma and renormalised at the
    map's edges (kind "gauss"), or with the aperture-mass filter (1 - r^2 / 2 s^2) exp(-r^2 / 2 s^2) / (2 pi s^2) built
    from it (kind "map"), on the device of `slicer`, on its stream.  The map does not wrap;
    radius is the filter's reach in pixels."""
    _handle, _destroy = "_sh", "slicer_smooth_destroy"
    _run, _run_npix = "slicer_smooth_run", "slicer_smooth_run_npix"

    def __init__(self, slicer: Slicer, npix, kind="gauss", sigma_pix=1.0, truncate=4.0):
        if kind not in _SMOOTH_KINDS:
            raise ValueError('kind: "gauss" or "map"')
        self._s = slicer
        self.npix, self.kind, self.sigma_pix, self.truncate = int(npix), kind, float(sigma_pix), float(truncate)
        self.last_npix = None  # of the last run
        sh = C.c_void_p()
        slicer._chk(_L.slicer_smooth_create(slicer._h, self.npix, _SMOOTH_KINDS[kind], self.sigma_pix, self.truncate,
                                            C.byref(sh)))
        self._sh = sh
        self.radius = smooth_weights(self.sigma_pix, self.truncate)[0]

    def device_map(self):
        """Device address of the last run's output, f32 [n, n] for the n of that run."""
        p = C.c_void_p()
        self._s._chk(_L.slicer_smooth_device_map(self._sh, C.byref(p)))
        return p.value

    def read(self):
        """The last run's output, f32 [n, n] for the n of that run; waits for the stream."""
        n = self.last_npix or 1
        out = np.empty((n, n), np.float32)
        self._s._chk(_L.slicer_smooth_read(self._sh, out.ctypes.data))
        return out


def noise_words(seed, stream, realisation, block):
    """The four Philox4x32-10 words (uint32 [4]) of block `block` of (seed, stream, realisation), as slicer_noise_words
    makes them; host only, no device needed."""
    w = np.empty(4, np.uint32)
    _host_chk(_L.slicer_noise_words(int(seed), int(stream), int(realisation), int(block), w.ctypes.data))
    return w


def noise_sigma_pix(sigma_e, ngal_arcmin2, angle_deg, npix):
    """sigma_e / sqrt(n_gal A_pix), A_pix = (60 angle_deg / npix)^2 arcmin^2: the shape noise of a pixel for an
    ellipticity dispersion sigma_e PER COMPONENT and n_gal galaxies per arcmin^2; host only, no device needed."""
    out = C.c_double()
    _host_chk(_L.slicer_noise_sigma_pix(float(sigma_e), float(ngal_arcmin2), float(angle_deg), int(npix), C.byref(out)))
    return out.value


def smooth_noise_gain(kind, sigma_pix, truncate=4.0):
    """The rms of Smooth's output for white noise of unit variance, at a pixel at least the radius away from every edge
    (slicer_smooth_noise_gain): sigma_smoothed = sigma_pix_noise * gain; host only, no device needed."""
    if kind not in _SMOOTH_KINDS:
        raise ValueError('kind: "gauss" or "map"')
    out = C.c_double()
    _host_chk(_L.slicer_smooth_noise_gain(_SMOOTH_KINDS[kind], float(sigma_pix), float(truncate), C.byref(out)))
    return out.value


class Noise(_SubHandle):
    """Shape noise for maps of up to npix^2 pixels on the device of `slicer`, on its stream:
    out = x + sigma z, z standard normals that are a pure function of (seed, stream, realisation, flat pixel index)."""
    _handle, _destroy = "_nh", "slicer_noise_destroy"

    def __init__(self, slicer: Slicer, npix, seed=0):
        self._s = slicer
        self.npix, self.seed = int(npix), int(seed)
        self.last_shape = None  # of the last run
        nh = C.c_void_p()
        slicer._chk(_L.slicer_noise_create(slicer._h, self.npix, self.seed, C.byref(nh)))
        self._nh = nh

    def run(self, d_map=None, sigma=1.0, stream=0, realisation=0, npix=None):
        """d_map: device address of an f32 map of npix^2 pixels (None: the handle's npix; otherwise at most that), or
        None for the noise alone; it may be device_map() itself (a second layer)."""
        d = None if d_map is None else int(d_map)
        if npix is None:
            self._s._chk(_L.slicer_noise_run(self._nh, d, float(sigma), int(stream), int(realisation)))
        else:
            self._s._chk(_L.slicer_noise_run_npix(self._nh, d, int(npix), float(sigma), int(stream), int(realisation)))
        n = self.npix if npix is None else int(npix)
        self.last_shape = (n, n)

    def run_at(self, d_map, first_pixel, count, sigma=1.0, stream=0, realisation=0):
        """The pixels first_pixel ... first_pixel + count - 1 of the flat index (first_pixel a multiple of 4); d_map
        (or None) and the output both start at that pixel."""
        d = None if d_map is None else int(d_map)
        self._s._chk(_L.slicer_noise_run_at(self._nh, d, int(first_pixel), int(count), float(sigma), int(stream),
                                            int(realisation)))
        self.last_shape = (int(count),)

    def run_kappa(self, kappa: Kappa, s, sigma=1.0, stream=0, realisation=0):
        """The map of source s of a Kappa accumulator, where it is."""
        self.run(kappa.device_map(s), sigma, stream, realisation, kappa.npix)

    def run_level(self, moments: Moments, level, sigma=1.0, stream=0, realisation=0):
        """Level `level` >= 1 of the last run of a Moments pyramid, where it is (level 0 is the caller's own map)."""
        self.run(moments.device_map(level), sigma, stream, realisation, moments.npix >> int(level))

    def words(self, first_block, n_blocks, stream=0, realisation=0):
        """The words of blocks first_block ... first_block + n_blocks - 1 as the device makes them, uint32 [n_blocks, 4]."""
        n_blocks = int(n_blocks)
        d = self._s.malloc(16 * max(n_blocks, 1))
        try:
            self._s._chk(_L.slicer_noise_words_device(self._nh, int(first_block), n_blocks, int(stream), int(realisation), d))
            return self._s.to_host(d, (n_blocks, 4), np.uint32)
        finally:
            self._s.free(d)

    def device_map(self):
        """Device address of the last run's output: f32, the pixels of that run."""
        p = C.c_void_p()
        self._s._chk(_L.slicer_noise_device_map(self._nh, C.byref(p)))
        return p.value

    def read(self):
        """The last run's output: f32 [n, n] after run, [count] after run_at; waits for the stream."""
        out = np.empty(self.last_shape or (1,), np.float32)
        self._s._chk(_L.slicer_noise_read(self._nh, out.ctypes.data))
        return out


STARLET_MAX_SCALES = 12


def starlet_gains(scales):
    """(gain_w [scales], gain_coarse) as slicer_starlet_gains makes them: the rms of w_1 ... w_scales and of the coarse
    map of Starlet for white noise of unit variance, at a pixel farther than the reach from every edge; host only, no
    device needed."""
    scales = int(scales)
    g = np.zeros(max(scales, 0), np.float64)
    coarse = C.c_double()
    _host_chk(_L.slicer_starlet_gains(scales, g.ctypes.data, C.byref(coarse)))
    return g, coarse.value


class Starlet(_MapRuns, _SubHandle):
    """The starlet transform (isotropic undecimated wavelet transform, B3-spline a trous, mirrored edges) of an npix^2
    map into `scales` wavelet maps w_1 ... w_J and one coarse map that sum back to it, on the device of `slicer`, on its
    stream.  Scale j reaches 2 * 2^j pixels; scale 0 names the coarse map."""
    _handle, _destroy = "_sh", "slicer_starlet_destroy"
    _run, _run_npix = "slicer_starlet_run", "slicer_starlet_run_npix"

    def __init__(self, slicer: Slicer, npix, scales):
        self._s = slicer
        self.npix, self.scales = int(npix), int(scales)
        self.last_npix = None  # of the last run
        sh = C.c_void_p()
        slicer._chk(_L.slicer_starlet_create(slicer._h, self.npix, self.scales, C.byref(sh)))
        self._sh = sh

    def device_map(self, scale):
        """Device address of w_scale (1 ... scales) or of the coarse map (0) of the last run, f32 [n, n] for its n."""
        p = C.c_void_p()
        self._s._chk(_L.slicer_starlet_device_map(self._sh, int(scale), C.byref(p)))
        return p.value

    def read(self, scale):
        """w_scale (1 ... scales) or the coarse map (0) of the last run, f32 [n, n] for its n; waits for the stream."""
        n = self.last_npix or 1
        out = np.empty((n, n), np.float32)
        self._s._chk(_L.slicer_starlet_read(self._sh, int(scale), out.ctypes.data))
        return out

    def read_all(self):
        """[coarse, w_1, ..., w_scales] of the last run: read(0) ... read(scales)."""
        return [self.read(j) for j in range(self.scales + 1)]


class L1Norm(_MapRuns, _SubHandle):
    """Per bin of the f64 `edges` (Peaks' rule: the last bin closed) the exact int64 count of an npix^2 map's pixels
    and the f64 sum of their |x|, on the device of `slicer`, on its stream: on the scales of a
    Starlet, the starlet l1-norm."""
    _handle, _destroy = "_lh", "slicer_l1norm_destroy"
    _run, _run_npix = "slicer_l1norm_run", "slicer_l1norm_run_npix"

    def __init__(self, slicer: Slicer, npix, edges):
        self._s = slicer
        self.npix = int(npix)
        self.edges = np.array(edges, np.float64).ravel()
        self.n_bins = self.edges.size - 1
        lh = C.c_void_p()
        slicer._chk(_L.slicer_l1norm_create(slicer._h, self.npix, self.edges.size, _dptr(self.edges), C.byref(lh)))
        self._lh = lh

    def run_scale(self, starlet: Starlet, scale):
        """Scale `scale` of the last run of a Starlet, where it is."""
        self.run(starlet.device_map(scale), starlet.last_npix)

    def read(self):
        """dict: edges [B+1], counts (int64 [B]), l1 (f64 [B]: the sums of |x|), below, above, nan (int) and below_l1,
        above_l1 (float)."""
        B = max(self.n_bins, 0)
        counts, l1 = np.empty(B, np.int64), np.empty(B, np.float64)
        below, above, nan = (np.empty(1, np.int64) for _ in range(3))
        below_l1, above_l1 = np.empty(1, np.float64), np.empty(1, np.float64)
        self._s._chk(_L.slicer_l1norm_read(self._lh, counts.ctypes.data, l1.ctypes.data, below.ctypes.data,
                                           above.ctypes.data, nan.ctypes.data, below_l1.ctypes.data, above_l1.ctypes.data))
        return {"edges": self.edges.copy(), "counts": counts, "l1": l1, "below": int(below[0]), "above": int(above[0]),
                "nan": int(nan[0]), "below_l1": float(below_l1[0]), "above_l1": float(above_l1[0])}


PCL_MAX_BINS = 512


def pcl_taper(npix, width_pix):
    """The border taper table f [npix] (f64) as slicer_pcl_taper makes it: with x_i = min(i, npix-1-i) + 0.5 and
    t = x_i / width_pix, f_i = 1 for t >= 1, else t - sin(2 pi t) / (2 pi); host only, no device needed."""
    f = np.zeros(max(int(npix), 0), np.float64)
    _host_chk(_L.slicer_pcl_taper(int(npix), float(width_pix), f.ctypes.data))
    return f


class Pcl(_SubHandle):
    """Masked pseudo-C_l of n_maps npix^2 maps of side angle_deg degrees under one shared mask, on the device of
    `slicer`, on its stream: the coupled bandpowers of the masked maps, the mode-coupling matrix
    of the mask and the decoupled bandpowers.  cross and the edges (required; units of l_f, or ell_edges in multipoles;
    at most 512 bins) as for Power."""
    _handle, _destroy = "_ph", "slicer_pcl_destroy"

    def __init__(self, slicer: Slicer, npix, angle_deg, n_maps, cross=False, edges=None, ell_edges=None):
        self._s = slicer
        self.npix, self.angle_deg, self.n_maps, self.cross = int(npix), float(angle_deg), int(n_maps), bool(cross)
        ok = math.isfinite(self.angle_deg) and self.angle_deg > 0  # otherwise slicer_pcl_create refuses it
        self.ell_f = ell_fundamental(self.angle_deg) if ok else math.nan
        if edges is None and ell_edges is None:
            raise ValueError("Pcl needs edges or ell_edges")
        n_edges, e = _edges(self.npix, edges, ell_edges, self.angle_deg)
        self.edges = e.copy()
        self.n_bins = n_edges - 1
        ph = C.c_void_p()
        slicer._chk(_L.slicer_pcl_create(slicer._h, self.npix, self.angle_deg, self.n_maps, int(self.cross), n_edges,
                                         _dptr(e), C.byref(ph)))
        self._ph = ph

    def set_mask(self, d_mask=None, taper_pix=0.0):
        """d_mask: device address of an f32 npix^2 mask, or None for the border taper alone; taper_pix: the taper's
        width in pixels, 0 for the mask alone.  Builds the coupling matrix; waits for the stream."""
        self._s._chk(_L.slicer_pcl_set_mask(self._ph, None if d_mask is None else int(d_mask), float(taper_pix)))

    def mask(self):
        """The mask in use, f32 [npix, npix]."""
        out = np.empty((self.npix, self.npix), np.float32)
        self._s._chk(_L.slicer_pcl_read_mask(self._ph, out.ctypes.data))
        return out

    def coupling(self):
        """dict: M [B, B] (rows and columns of empty bins are 0), mean_w, mean_w2."""
        B = max(self.n_bins, 0)
        M = np.empty((B, B), np.float64)
        m1, m2 = C.c_double(), C.c_double()
        self._s._chk(_L.slicer_pcl_coupling(self._ph, M.ctypes.data, C.byref(m1), C.byref(m2)))
        return {"M": M, "mean_w": m1.value, "mean_w2": m2.value}

    def run(self, ptrs):
        """ptrs: device addresses of the n_maps f32 npix^2 maps (unmasked: the mask is applied as they are loaded)."""
        ptrs = [int(p) for p in ptrs]
        if len(ptrs) != self.n_maps:
            raise ValueError(f"expected {self.n_maps} maps, got {len(ptrs)}")
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._s._chk(_L.slicer_pcl_run(self._ph, arr))

    def run_kappa(self, kappa: Kappa):
        """The maps of every source of a Kappa accumulator, where they are."""
        self.run([kappa.device_map(s) for s in range(kappa.n_sources)])

    def spectrum(self, map):
        """rfft2 of the masked map `map` of the last run, [npix, npix // 2 + 1] complex128 (auto mode: the last only)."""
        out = np.empty((self.npix, self.npix // 2 + 1), np.complex128)
        self._s._chk(_L.slicer_pcl_spectrum(self._ph, int(map), out.ctypes.data))
        return out

    def read(self):
        """dict: ell_lo, ell_hi, ell (mean l), counts, and cl (decoupled; NaN in empty bins) and coupled, each
        [S][S][B], symmetric (cross) or [S][B] (auto)."""
        S, B = self.n_maps, self.n_bins
        npairs = S * (S + 1) // 2 if self.cross else S
        flat, cflat = np.empty((npairs, B), np.float64), np.empty((npairs, B), np.float64)
        ell = np.empty(B, np.float64)
        counts = np.empty(B, np.int64)
        self._s._chk(_L.slicer_pcl_read(self._ph, flat.ctypes.data, cflat.ctypes.data, ell.ctypes.data,
                                        counts.ctypes.data))

        def square(x):
            if not self.cross:
                return x
            out = np.empty((S, S, B), np.float64)
            p = 0
            for s in range(S):
                for t in range(s, S):
                    out[s, t] = out[t, s] = x[p]
                    p += 1
            return out
        return {"ell_lo": self.edges[:-1] * self.ell_f, "ell_hi": self.edges[1:] * self.ell_f, "ell": ell,
                "counts": counts, "cl": square(flat), "coupled": square(cflat)}


PCL2_MAX_BINS = 128
PCL2_E, PCL2_B, PCL2_KAPPA = 0, 1, 2


def spin_phases(npix, spin):
    """(C, S), each f64 [npix, npix // 2 + 1]: cos and sin of spin (2 or 4) times the mode's polar angle as
    slicer_pcl2_phases makes them (the sines 0 on the Nyquist lines of an even npix); host only, no device needed."""
    n = max(int(npix), 0)
    c, s = np.zeros((n, n // 2 + 1), np.float64), np.zeros((n, n // 2 + 1), np.float64)
    _host_chk(_L.slicer_pcl2_phases(int(npix), int(spin), c.ctypes.data, s.ctypes.data))
    return c, s


class PclShear(_SubHandle):
    """E/B pseudo-C_l of n_fields masked shear fields (gamma1, gamma2; with_kappa: and kappa) of npix^2 pixels and side
    angle_deg degrees under one shared mask, on the device of `slicer`, on its stream: the
    coupled bandpowers of E, B and kappa, the coupling matrices M0, M2, X2, M4, X4 of the mask and the bandpowers
    decoupled by their block systems.  cross: all pairs of fields, else the pairs within each field.  The edges
    (required; units of l_f, or ell_edges in multipoles) as for Pcl, at most 128 bins."""
    _handle, _destroy = "_ph", "slicer_pcl2_destroy"

    def __init__(self, slicer: Slicer, npix, angle_deg, n_fields, with_kappa=False, cross=False, edges=None,
                 ell_edges=None):
        self._s = slicer
        self.npix, self.angle_deg, self.n_fields = int(npix), float(angle_deg), int(n_fields)
        self.with_kappa, self.cross = bool(with_kappa), bool(cross)
        self.n_comp = 3 if self.with_kappa else 2  # per field
        ok = math.isfinite(self.angle_deg) and self.angle_deg > 0  # otherwise slicer_pcl2_create refuses it
        self.ell_f = ell_fundamental(self.angle_deg) if ok else math.nan
        if edges is None and ell_edges is None:
            raise ValueError("PclShear needs edges or ell_edges")
        n_edges, e = _edges(self.npix, edges, ell_edges, self.angle_deg)
        self.edges = e.copy()
        self.n_bins = n_edges - 1
        ph = C.c_void_p()
        slicer._chk(_L.slicer_pcl2_create(slicer._h, self.npix, self.angle_deg, self.n_fields, int(self.with_kappa),
                                          int(self.cross), n_edges, _dptr(e), C.byref(ph)))
        self._ph = ph

    def set_mask(self, d_mask=None, taper_pix=0.0):
        """As Pcl.set_mask; builds the five coupling matrices and the three block systems; waits for the stream."""
        self._s._chk(_L.slicer_pcl2_set_mask(self._ph, None if d_mask is None else int(d_mask), float(taper_pix)))

    def mask(self):
        """The mask in use, f32 [npix, npix]."""
        out = np.empty((self.npix, self.npix), np.float32)
        self._s._chk(_L.slicer_pcl2_read_mask(self._ph, out.ctypes.data))
        return out

    def coupling(self):
        """dict: M0, M2, X2, M4, X4, each [B, B] (rows and columns of empty bins are 0), mean_w, mean_w2."""
        B = max(self.n_bins, 0)
        m = {k: np.empty((B, B), np.float64) for k in ("M0", "M2", "X2", "M4", "X4")}
        m1, m2 = C.c_double(), C.c_double()
        self._s._chk(_L.slicer_pcl2_coupling(self._ph, *(a.ctypes.data for a in m.values()), C.byref(m1), C.byref(m2)))
        m.update(mean_w=m1.value, mean_w2=m2.value)
        return m

    def run(self, ptrs):
        """ptrs: device addresses of the f32 npix^2 maps, per field gamma1, gamma2 and, with kappa, kappa (unmasked)."""
        ptrs = [int(p) for p in ptrs]
        if len(ptrs) != self.n_fields * self.n_comp:
            raise ValueError(f"expected {self.n_fields * self.n_comp} maps, got {len(ptrs)}")
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._s._chk(_L.slicer_pcl2_run(self._ph, arr))

    def run_shear(self, shears, kappas=None):
        """The gamma1, gamma2 device maps of the last run of every Shear handle in `shears`, where they are; kappas:
        with kappa, the device address of each field's kappa map."""
        ptrs = []
        for f, sh in enumerate(shears):
            ptrs += [sh.device_map(SHEAR_GAMMA1), sh.device_map(SHEAR_GAMMA2)]
            if self.with_kappa:
                ptrs.append(kappas[f])
        self.run(ptrs)

    def spectrum(self, field, comp):
        """The spectrum of component comp (0, 1, 2 = E, B, kappa) of field `field` of the last run,
        [npix, npix // 2 + 1] complex128 (auto mode: the last field only)."""
        out = np.empty((self.npix, self.npix // 2 + 1), np.complex128)
        self._s._chk(_L.slicer_pcl2_spectrum(self._ph, int(field), int(comp), out.ctypes.data))
        return out

    def read(self):
        """dict: ell_lo, ell_hi, ell (mean l), counts, and `cl` (decoupled; NaN in empty bins) and `coupled`, each a
        dict of named arrays EE, EB, BE, BB and, with kappa, kE, kB, Ek, Bk, kk: XY[f][g][B] is component X of field f
        against component Y of field g (cross), or XY[f][B] within field f (auto)."""
        F, B, nc = self.n_fields, self.n_bins, self.n_comp
        S = F * nc
        npairs = S * (S + 1) // 2 if self.cross else F * (nc * (nc + 1) // 2)
        flat, cflat = np.empty((npairs, B), np.float64), np.empty((npairs, B), np.float64)
        ell = np.empty(B, np.float64)
        counts = np.empty(B, np.int64)
        self._s._chk(_L.slicer_pcl2_read(self._ph, flat.ctypes.data, cflat.ctypes.data, ell.ctypes.data,
                                         counts.ctypes.data))

        def pair(i, j, n):
            i, j = min(i, j), max(i, j)
            return i * n - i * (i - 1) // 2 + (j - i)

        def named(x):
            out = {}
            for a, la in enumerate("EBk"[:nc]):
                for b, lb in enumerate("EBk"[:nc]):
                    if self.cross:
                        v = np.empty((F, F, B), np.float64)
                        for f in range(F):
                            for g in range(F):
                                v[f, g] = x[pair(f * nc + a, g * nc + b, S)]
                    else:
                        v = np.empty((F, B), np.float64)
                        for f in range(F):
                            v[f] = x[f * (nc * (nc + 1) // 2) + pair(a, b, nc)]
                    out[la + lb] = v
            return out
        return {"ell_lo": self.edges[:-1] * self.ell_f, "ell_hi": self.edges[1:] * self.ell_f, "ell": ell,
                "counts": counts, "cl": named(flat), "coupled": named(cflat)}


XI_MAX_BINS = 512
XI_PLUS, XI_MINUS, XI_CROSS, XI_WEIGHTS = range(4)


def xi_bins(npix, edges):
    """Host only (no device): {"counts": N_b, "lags": M_b (int64 each), "padded": P} for edges in pixels, as
    slicer_xi_bins enumerates them."""
    e = np.ascontiguousarray(edges, np.float64).ravel()
    B = max(e.size - 1, 0)
    counts, lags = np.zeros(B, np.int64), np.zeros(B, np.int64)
    P = C.c_int32()
    _host_chk(_L.slicer_xi_bins(int(npix), e.size, _dptr(e), counts.ctypes.data, lags.ctypes.data, C.byref(P)))
    return {"counts": counts, "lags": lags, "padded": P.value}


class Xi(_SubHandle):
    """Real-space two-point correlation functions of n_fields npix^2 fields under one shared weight map, on the device
    of `slicer`, on its stream.  spin=0: xi_ab(theta) of maps; spin=2: xi+ and xi- of (gamma1,
    gamma2) pairs.  cross=False: every field with itself; cross=True: every pair.  edges in pixels (required; at most
    512 bins).  The maps are not periodic: nothing wraps, and any weight map is divided out exactly."""
    _handle, _destroy = "_xh", "slicer_xi_destroy"

    def __init__(self, slicer: Slicer, npix, spin, n_fields, edges, cross=False):
        self._s = slicer
        self.npix, self.spin, self.n_fields, self.cross = int(npix), int(spin), int(n_fields), bool(cross)
        self.edges = np.ascontiguousarray(edges, np.float64).ravel().copy()
        self.n_bins = self.edges.size - 1
        self.n_pairs = self.n_fields * (self.n_fields + 1) // 2 if self.cross else self.n_fields
        xh = C.c_void_p()
        slicer._chk(_L.slicer_xi_create(slicer._h, self.npix, self.spin, self.n_fields, int(self.cross), self.edges.size,
                                        _dptr(self.edges), C.byref(xh)))
        self._xh = xh
        self.max_lag = min(int(math.ceil(self.edges[-1])), self.npix - 1)

    def set_weights(self, d_w=None):
        """d_w: device address of an f32 npix^2 weight map (finite, >= 0), or None for w = 1.  Waits for the stream."""
        self._s._chk(_L.slicer_xi_set_weights(self._xh, None if d_w is None else int(d_w)))

    def run(self, ptrs):
        """ptrs: device addresses of the f32 npix^2 maps: n_fields of them (spin 0), or gamma1, gamma2 of field 0, then
        of field 1, ... (spin 2)."""
        ptrs = [int(p) for p in ptrs]
        want = self.n_fields * (2 if self.spin else 1)
        if len(ptrs) != want:
            raise ValueError(f"expected {want} maps, got {len(ptrs)}")
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        self._s._chk(_L.slicer_xi_run(self._xh, arr))

    def run_kappa(self, kappa: Kappa):
        """Spin 0: the maps of every source of a Kappa accumulator, where they are."""
        self.run([kappa.device_map(s) for s in range(kappa.n_sources)])

    def read(self):
        """dict: r_lo, r_hi (bin edges in pixels), r (the weighted mean lag), weights (W_b), counts (N_b), and xi (spin
        2: xip and xim), each [F][F][B], symmetric (cross) or [F][B] (auto); NaN in empty bins."""
        F, B = self.n_fields, self.n_bins
        flat = np.empty((self.n_pairs, B), np.float64)
        mflat = np.empty((self.n_pairs, B), np.float64) if self.spin else None
        r, W = np.empty(B, np.float64), np.empty(B, np.float64)
        counts = np.empty(B, np.int64)
        self._s._chk(_L.slicer_xi_read(self._xh, flat.ctypes.data, _dptr(mflat), r.ctypes.data, W.ctypes.data,
                                       counts.ctypes.data))

        def square(x):
            if not self.cross:
                return x
            out = np.empty((F, F, B), np.float64)
            p = 0
            for s in range(F):
                for t in range(s, F):
                    out[s, t] = out[t, s] = x[p]
                    p += 1
            return out
        out = {"r_lo": self.edges[:-1].copy(), "r_hi": self.edges[1:].copy(), "r": r, "weights": W, "counts": counts}
        if self.spin:
            out["xip"], out["xim"] = square(flat), square(mflat)
        else:
            out["xi"] = square(flat)
        return out

    def correlation(self, pair=0, which=XI_PLUS):
        """The lag window of one inverse of pair `pair` (pair-major, as read's flat order) of the last run, f64
        [2L+1, 2L+1] indexed [dx + L, dy + L]: XI_PLUS, XI_MINUS, XI_CROSS, or XI_WEIGHTS for W(r)."""
        W = 2 * self.max_lag + 1
        out = np.empty((W, W), np.float64)
        self._s._chk(_L.slicer_xi_correlation(self._xh, int(pair), int(which), out.ctypes.data))
        return out


SCATTERING_MAX_J = 12
SCATTERING_MAX_L = 16


def scattering_filter(npix, J, L, j, l):
    """Host only (no device): the Morlet filter psi^_{jl} of the scattering bank over the full mode plane, f64
    [npix, npix], as slicer_scattering_filter defines it."""
    out = np.empty((int(npix), int(npix)) if npix > 0 else (0, 0), np.float64)
    _host_chk(_L.slicer_scattering_filter(int(npix), int(J), int(L), int(j), int(l), out.ctypes.data))
    return out


def scattering_reduce(s1, s2):
    """numpy only: the orientation averages of Scattering.read's s1 [J, L] and s2 [J, L, J, L]: s1(j) [J] and
    s2(j1, j2, (l2 - l1) mod L) [J, J, L], NaN where j2 <= j1."""
    s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
    J, L = s1.shape
    if s2.shape != (J, L, J, L):
        raise ValueError(f"s2 has shape {s2.shape}, expected {(J, L, J, L)}")
    l1 = np.arange(L)
    r2 = np.stack([s2[:, l1, :, (l1 + d) % L].mean(axis=0) for d in range(L)], axis=-1)
    return s1.mean(axis=1), r2


class Scattering(_SubHandle):
    """Wavelet scattering coefficients of an npix^2 kappa map, orders 0, 1 and 2, over J dyadic scales and L
    orientations of Morlet filters, on the device of `slicer`, on its stream.  The map is taken
    as periodic; nothing is subsampled."""
    _handle, _destroy = "_sh", "slicer_scattering_destroy"

    def __init__(self, slicer: Slicer, npix, J, L):
        self._s = slicer
        self.npix, self.J, self.L = int(npix), int(J), int(L)
        sh = C.c_void_p()
        slicer._chk(_L.slicer_scattering_create(slicer._h, self.npix, self.J, self.L, C.byref(sh)))
        self._sh = sh

    def run(self, d_map):
        """d_map: device address of an f32 npix^2 map.  Enqueued."""
        self._s._chk(_L.slicer_scattering_run(self._sh, None if d_map is None else int(d_map)))

    def run_kappa(self, kappa: Kappa, s):
        """The map of source s of a Kappa accumulator, where it is."""
        self.run(kappa.device_map(s))

    def read(self):
        """dict: s0 [2] (the mean of kappa and of kappa^2), s1 and p1 [J, L] (the mean of u1 and of u1^2), s2
        [J, L, J, L] indexed [j1, l1, j2, l2], NaN where j2 <= j1."""
        J, L = self.J, self.L
        out = {"s0": np.empty(2, np.float64), "s1": np.empty((J, L), np.float64), "p1": np.empty((J, L), np.float64),
               "s2": np.empty((J, L, J, L), np.float64)}
        self._s._chk(_L.slicer_scattering_read(self._sh, *(out[k].ctypes.data for k in ("s0", "s1", "p1", "s2"))))
        return out

    def modulus(self, d_map, j1, l1, j2=-1, l2=-1):
        """The f64 [npix, npix] field u1 = W_{j1 l1} kappa, or W_{j2 l2} u1 with j2 > j1, recomputed from d_map."""
        out = np.empty((self.npix, self.npix), np.float64)
        self._s._chk(_L.slicer_scattering_modulus(self._sh, None if d_map is None else int(d_map), int(j1), int(l1),
                                                  int(j2), int(l2), out.ctypes.data))
        return out


RAYS_KAPPA, RAYS_GAMMA1, RAYS_GAMMA2, RAYS_OMEGA, RAYS_DEFLECTION1, RAYS_DEFLECTION2 = range(6)
RAYS_COUNT = 6
RAYS_STATE = ("b1", "b2", "t1", "t2", "A11", "A12", "A21", "A22", "T11", "T12", "T21", "T22")


class Rays(_SubHandle):
    """One ray per pixel of an npix^2 grid of `spacing` radians per pixel, traced through lens planes on the device of
    `slicer`, on its stream.  step takes a plane's five device maps; observe gives the
    distortion (kappa, gamma1, gamma2, omega) and the total deflection at a source distance."""
    _handle, _destroy = "_rh", "slicer_rays_destroy"

    def __init__(self, slicer: Slicer, npix, spacing):
        self._s = slicer
        self.npix, self.spacing = int(npix), float(spacing)
        rh = C.c_void_p()
        slicer._chk(_L.slicer_rays_create(slicer._h, self.npix, self.spacing, C.byref(rh)))
        self._rh = rh

    def reset(self):
        """Back to the start state."""
        self._s._chk(_L.slicer_rays_reset(self._rh))

    def step(self, chi, d_alpha1, d_alpha2, d_kappa, d_gamma1, d_gamma2):
        """Through the plane at comoving distance chi; the five arguments are device addresses of f32 npix^2 maps."""
        ptrs = [None if p is None else int(p) for p in (d_alpha1, d_alpha2, d_kappa, d_gamma1, d_gamma2)]
        self._s._chk(_L.slicer_rays_step(self._rh, float(chi), *ptrs))

    def step_shear(self, shear: Shear, chi, gradient=False, d_kappa=None):
        """The plane whose lens map was the last shear.run(d_kappa), followed by shear.deflection() (spectral maps) or
        shear.fd() (gradient=True: the finite-difference maps, which bring their own kappa)."""
        if gradient:
            maps = [shear.device_map(w) for w in (SHEAR_FD_ALPHA1, SHEAR_FD_ALPHA2, SHEAR_FD_KAPPA, SHEAR_FD_GAMMA1,
                                                  SHEAR_FD_GAMMA2)]
        else:
            if d_kappa is None:
                d_kappa = shear.last_input
            if d_kappa is None:
                raise ValueError("step_shear: the Shear handle has not run")
            maps = [shear.device_map(SHEAR_ALPHA1), shear.device_map(SHEAR_ALPHA2), d_kappa,
                    shear.device_map(SHEAR_GAMMA1), shear.device_map(SHEAR_GAMMA2)]
        self.step(chi, *maps)

    def observe_device(self, chi_s, ptrs):
        """slicer_rays_observe as it is: ptrs are RAYS_COUNT device addresses of npix^2 f32 buffers, None to skip one."""
        arr = (C.c_void_p * RAYS_COUNT)(*[None if p is None else int(p) for p in ptrs])
        self._s._chk(_L.slicer_rays_observe(self._rh, float(chi_s), arr))

    def observe(self, chi_s, which=tuple(range(RAYS_COUNT))):
        """{code: f32 [npix, npix] array} for the RAYS_* codes in `which`, for a source at comoving distance chi_s."""
        return _read_outputs(self._s, self.npix, which, RAYS_COUNT, "RAYS_*",
                             lambda ptrs: self.observe_device(chi_s, ptrs))

    def state(self):
        """The state, f64 [12, npix, npix] in the order of RAYS_STATE; waits for the stream."""
        out = np.empty((len(RAYS_STATE), self.npix, self.npix), np.float64)
        self._s._chk(_L.slicer_rays_state(self._rh, out.ctypes.data))
        return out

    def planes(self):
        """(number of steps since the start state, comoving distance of the last plane)."""
        n, chi = C.c_int32(), C.c_double()
        self._s._chk(_L.slicer_rays_planes(self._rh, C.byref(n), C.byref(chi)))
        return n.value, chi.value
