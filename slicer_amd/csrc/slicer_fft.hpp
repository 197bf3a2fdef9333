// slicer_fft.hpp -- internal (not exported): the forward f64 r2c transform of slicer_shear.hip, shared by the shear
// handle and the power-spectrum handle (row N7).  One plan per map size and shear_split value:
// the twiddles, the row and column pass chains, and the buffers the forward passes go through.
#pragma once

#include <hip/hip_runtime.h>

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
SLICER_FFT_INTERNAL void slicer_fft_destroy(slicer_fft_s *f);
