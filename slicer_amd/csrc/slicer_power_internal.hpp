// slicer_power_internal.hpp -- internal (not exported): what slicer_power.hip shares with the handles built on its
// bins: pseudo-C_l (slicer_pcl.hip, slicer_pcl_shear.hip), bispectrum (slicer_bispectrum.hip) and xi (slicer_xi.hip).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "slicer_fft.hpp"

// slicer_power_run with the maps multiplied by the f32 mask d_w on their way in (slicer_fft_forward_masked).
SLICER_FFT_INTERNAL int slicer_power_run_masked(slicer_power_handle ph, const float *const *d_maps, const float *d_w);
SLICER_FFT_INTERNAL slicer_fft_s *slicer_power_plan(slicer_power_handle ph);
// slicer_power_run_masked of a cross handle in its two halves, for a caller that changes the stored spectra in between
// (the E/B rotation of slicer_pcl_shear.hip); all enqueued on st.  slicer_power_transform_masked: the spectrum of map
// `s` = rfft2(d_w * d_map), and the handle has no run until the next slicer_power_bin_stored.  slicer_power_stored:
// where that spectrum lies, [n][n/2+1].  slicer_power_bin_stored: the binning and finish of slicer_power_run over
// the n_maps stored spectra, after which slicer_power_read and slicer_power_spectrum serve them; d_copy (or NULL)
// receives the [pairs][B] bandpowers as well.
SLICER_FFT_INTERNAL int slicer_power_transform_masked(slicer_power_handle ph, hipStream_t st, int s, const float *d_map,
                                                      const float *d_w);
SLICER_FFT_INTERNAL double2 *slicer_power_stored(slicer_power_handle ph, int s);
SLICER_FFT_INTERNAL int slicer_power_bin_stored(slicer_power_handle ph, hipStream_t st, double *d_copy);
// d_out[column * B + b] = norm / N_b * (sum of Re spec over the half-plane modes of bin b), NaN for an empty bin: the
// binning of slicer_power_run (same slices, same summation order) of the real parts; enqueued on st.
SLICER_FFT_INTERNAL int slicer_power_bin_real(slicer_power_handle ph, hipStream_t st, const double2 *spec, double norm,
                                              int column, double *d_out);
// The bin edges of slicer_power_bins into `out`, or 0 .. npix-1 for NULL (then n_edges must be npix); "" if they are
// usable, else why not.
SLICER_FFT_INTERNAL const char *check_edges(int npix, int n_edges, const double *edges, std::vector<double> &out);
// Smallest j in [0, cap] with a2 + j^2 >= e2 (strict: > e2), cap if none.  a2 + j^2 is an integer below 2^53, so the
// comparisons are exact; the square root only gives the starting point.  The bin walk of power and xi.
__host__ __device__ inline int first_at_least(double a2, double e2, bool strict, int cap)
{
    const double t = e2 - a2;
    int j;
    if (!(t > 0.0))
        j = 0;
    else if (t >= (double)cap * (double)cap)
        j = cap;
    else
        j = std::min(cap, (int)ceil(sqrt(t)));
    auto ok = [&](int x) {
        const double m = a2 + (double)x * (double)x;
        return strict ? m > e2 : m >= e2;
    };
    while (j > 0 && ok(j - 1))
        j--;
    while (j < cap && !ok(j))
        j++;
    return j;
}
