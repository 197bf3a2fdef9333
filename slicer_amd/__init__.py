"""slicer_amd -- MI355X-native particle->grid mass assignment (the SLICER densitymaps hot path).

Importing loads slicer_amd/libslicer_amd.so (HIP kernels + C ABI, include/slicer_amd.h) and fails
loudly if it is missing: there is no CPU fallback in this package.
"""
from . import _lib, gadget, synth  # noqa: F401
from .api import (ACC_F32, ACC_F64, ACC_FIXED64, ALGO_AUTO, ALGO_BINNED, ALGO_DIRECT, ELEM_F32, ELEM_F64,  # noqa: F401
                  ELEM_FIXED64, MAS_NGP, MAS_TSC, InputParams, Lens, Random, Slicer, SlicerError, createDensityMaps)

from .lensing import (FD_ALPHA1, FD_ALPHA2, FD_COUNT, FD_GAMMA, FD_GAMMA1, FD_GAMMA2, FD_KAPPA,  # noqa: F401
                      SHEAR_ALPHA1, SHEAR_ALPHA2, SHEAR_FD_ALPHA1, SHEAR_FD_ALPHA2, SHEAR_FD_GAMMA, SHEAR_FD_GAMMA1,
                      SHEAR_FD_GAMMA2, SHEAR_FD_KAPPA, SHEAR_GAMMA, SHEAR_GAMMA1, SHEAR_GAMMA2, SHEAR_PHI, Kappa, Power,
                      Shear, ell_fundamental, fd_derivatives, fd_run, plane_weights, power_bins, shear_supported)
from .lensing import HALVE_MEAN, HALVE_SUM, MOMENTS_ORDERS, Moments, combine_moments, moments_depth  # noqa: F401
from .lensing import PEAKS_MAX_BINS, Peaks, peaks_edges  # noqa: F401
from .lensing import MINKOWSKI_MAX_THRESHOLDS, Minkowski, minkowski_functionals  # noqa: F401
from .lensing import BISPECTRUM_MAX_BINS, Bispectrum, bispectrum_triangles, bispectrum_triples  # noqa: F401
from .lensing import SMOOTH_GAUSS, SMOOTH_MAP, SMOOTH_MAX_RADIUS, Smooth, smooth_weights  # noqa: F401
from .lensing import Noise, noise_sigma_pix, noise_words, smooth_noise_gain  # noqa: F401
from .lensing import STARLET_MAX_SCALES, L1Norm, Starlet, starlet_gains  # noqa: F401
from .lensing import PCL_MAX_BINS, Pcl, pcl_taper  # noqa: F401
from .lensing import PCL2_B, PCL2_E, PCL2_KAPPA, PCL2_MAX_BINS, PclShear, spin_phases  # noqa: F401
from .lensing import BETTI_MAX_NPIX, BETTI_MAX_THRESHOLDS, Betti  # noqa: F401
from .lensing import (CATALOGUE_DTYPE, CATALOGUE_FALLBACK, CATALOGUE_MAX_CAPACITY, CATALOGUE_MAX_NPIX,  # noqa: F401
                      CATALOGUE_MINIMA, CATALOGUE_MINIMUM, CATALOGUE_PEAKS, PeakCatalogue)
from .lensing import SCATTERING_MAX_J, SCATTERING_MAX_L, Scattering, scattering_filter, scattering_reduce  # noqa: F401
from .lensing import XI_CROSS, XI_MAX_BINS, XI_MINUS, XI_PLUS, XI_WEIGHTS, Xi, xi_bins  # noqa: F401
from .lensing import (RAYS_COUNT, RAYS_DEFLECTION1, RAYS_DEFLECTION2, RAYS_GAMMA1, RAYS_GAMMA2, RAYS_KAPPA,  # noqa: F401
                      RAYS_OMEGA, RAYS_STATE, Rays, plane_strengths)

__version__ = "0.2.0"
