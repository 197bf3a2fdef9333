// slicer_fft.hpp -- internal (not exported): the forward f64 r2c transform of slicer_shear.hip, shared by the shear
// handle, the power-spectrum handle (row N7), the bispectrum handle (row N15), the pseudo-C_l
// handle (row N17), the correlation-function handle (row N18) and the scattering handle (row N20).  One plan per map size and shear_split value:
// the twiddles, the row and column pass chains, and the buffers the forward passes go through.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/slicer_amd.h"

struct slicer_fft_s;

// Plans the transforms of npix^2 maps (fft_size_supported(npix); the caller checks) on `device`, the current device and
// that of st (sub_open), uploads the twiddles (waits for st) and allocates the row buffer and the pass intermediates.
// split: the shear_split option.  Errors go to h's slicer_last_error, prefixed with `who`.
#define SLICER_FFT_INTERNAL __attribute__((visibility("hidden")))
SLICER_FFT_INTERNAL int slicer_fft_create(slicer_handle h, int npix, int split, hipStream_t st, int device,
                                          const char *who, slicer_fft_s **out);
// khat = rfft2(map) in f64, [npix][npix/2+1] (re, im) pairs; enqueued on st.  khat is none of the plan's buffers.
SLICER_FFT_INTERNAL int slicer_fft_forward(slicer_fft_s *f, hipStream_t st, const float *map, double2 *khat);
// out = irfft2(khat * 1[mode in band]), s = (npix, npix), kept in f64: npix^2 doubles, none of the plan's buffers.  A
// mode is in the band iff lo2 <= m2 < hi2 on the exact integer m2 (m2 <= hi2 with closed != 0) and m2 != 0 (with
// keep_dc != 0, m2 = 0 is in the band like any other mode).  khat = NULL: the transform of the band's indicator itself.
// The inverse chain of the shear handle with a band load and an f64 store; enqueued on st.
SLICER_FFT_INTERNAL int slicer_fft_inverse_band(slicer_fft_s *f, hipStream_t st, const double2 *khat, double lo2,
                                                double hi2, int closed, double *out, int keep_dc = 0);
// The entry points of the masked pseudo-C_l handle (slicer_pcl.hip, row N17), all enqueued on st; none of their
// arguments is one of the plan's buffers.
// khat = rfft2(mask * map), the products taken in f32 (one rounding) as the rows are loaded: bitwise
// slicer_fft_forward of the multiplied map.
SLICER_FFT_INTERNAL int slicer_fft_forward_masked(slicer_fft_s *f, hipStream_t st, const float *map, const float *mask,
                                                  double2 *khat);
// khat = rfft2(x * y) for two f64 npix^2 maps, the products taken in f64 as the rows are loaded.
SLICER_FFT_INTERNAL int slicer_fft_forward_product(slicer_fft_s *f, hipStream_t st, const double *x, const double *y,
                                                   double2 *khat);
// khat = rfft2(sqrt(x * x + y * y)) for two f64 npix^2 maps, the modulus taken in f64 as the rows are loaded, rounded
// after every operation; it is never stored (the scattering handle, slicer_scattering.hip, row N20).
SLICER_FFT_INTERNAL int slicer_fft_forward_hypot(slicer_fft_s *f, hipStream_t st, const double *x, const double *y,
                                                 double2 *khat);
// out = irfft2(|khat|^2), s = (npix, npix), kept in f64: npix^2 doubles.
SLICER_FFT_INTERNAL int slicer_fft_inverse_abs2(slicer_fft_s *f, hipStream_t st, const double2 *khat, double *out);
SLICER_FFT_INTERNAL void slicer_fft_destroy(slicer_fft_s *f);
// Internal entry points of the power handle (slicer_power.hip) for the pseudo-C_l handle built on one.
// slicer_power_run with the maps multiplied by the f32 mask d_w on their way in (slicer_fft_forward_masked).
SLICER_FFT_INTERNAL int slicer_power_run_masked(slicer_power_handle ph, const float *const *d_maps, const float *d_w);
SLICER_FFT_INTERNAL slicer_fft_s *slicer_power_plan(slicer_power_handle ph);
// d_out[column * B + b] = norm / N_b * (sum of Re spec over the half-plane modes of bin b), NaN for an empty bin: the
// binning of slicer_power_run (same slices, same summation order) of the real parts; enqueued on st.
SLICER_FFT_INTERNAL int slicer_power_bin_real(slicer_power_handle ph, hipStream_t st, const double2 *spec, double norm,
                                              int column, double *d_out);
// The bin edges of slicer_power_bins into `out`, or 0 .. npix-1 for NULL (then n_edges must be npix); "" if they are
// usable, else why not (slicer_power.hip).
SLICER_FFT_INTERNAL const char *check_edges(int npix, int n_edges, const double *edges, std::vector<double> &out);
// Smallest j in [0, cap] with a2 + j^2 >= e2 (strict: > e2), cap if none.  a2 + j^2 is an integer below 2^53, so the
// comparisons are exact; the square root only gives the starting point.
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
