// slicer_power_internal.hpp -- internal (not exported): what slicer_power.hip shares with the handles built on its
// bins: pseudo-C_l (slicer_pcl.hip), bispectrum (slicer_bispectrum.hip) and xi (slicer_xi.hip).
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

#include "slicer_fft.hpp"

// slicer_power_run with the maps multiplied by the f32 mask d_w on their way in (slicer_fft_forward_masked).
SLICER_FFT_INTERNAL int slicer_power_run_masked(slicer_power_handle ph, const float *const *d_maps, const float *d_w);
SLICER_FFT_INTERNAL slicer_fft_s *slicer_power_plan(slicer_power_handle ph);
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
