// slicer_fft.hpp -- internal (not exported): the forward f64 r2c transform of slicer_shear.hip, shared by the shear
// handle, the power-spectrum handle (row N7) and the bispectrum handle (row N15).  One plan per map size and shear_split value:
// the twiddles, the row and column pass chains, and the buffers the forward passes go through.
#pragma once

#include <hip/hip_runtime.h>

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
// mode is in the band iff lo2 <= m2 < hi2 on the exact integer m2 (m2 <= hi2 with closed != 0) and m2 != 0.  khat =
// NULL: the transform of the band's indicator itself.  The inverse chain of the shear handle with a band load and an
// f64 store; enqueued on st.
SLICER_FFT_INTERNAL int slicer_fft_inverse_band(slicer_fft_s *f, hipStream_t st, const double2 *khat, double lo2,
                                                double hi2, int closed, double *out);
SLICER_FFT_INTERNAL void slicer_fft_destroy(slicer_fft_s *f);
// The bin edges of slicer_power_bins into `out`, or 0 .. npix-1 for NULL (then n_edges must be npix); "" if they are
// usable, else why not (slicer_power.hip).
SLICER_FFT_INTERNAL const char *check_edges(int npix, int n_edges, const double *edges, std::vector<double> &out);
