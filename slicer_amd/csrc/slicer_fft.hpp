// slicer_fft.hpp -- internal (not exported): the f64 real-to-complex transform of npix^2 maps and its inverse
// (slicer_fft.hip), shared by the handles of DESIGN.md S8 rows N6/N8, N7, N15, N17, N18, N20 and N21.  One plan per map size
// and shear_split value: the twiddles, the row and column pass chains, and the buffers the passes go through.  Every
// transform is enqueued on the caller's stream, and none of its arguments is one of the plan's buffers.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/slicer_amd.h"

#define SLICER_FFT_INTERNAL __attribute__((visibility("hidden")))

constexpr int kFftMaxN = 16384;  // the largest supported map side (fft_size_supported, slicer_host.hpp)

struct slicer_fft_s;

// Plans the transforms of npix^2 maps (fft_size_supported(npix); the caller checks) on `device`, the current device and
// that of st (sub_open), uploads the twiddles (waits for st) and allocates the row buffer and the pass intermediates.
// split: the shear_split option.  Errors go to h's slicer_last_error, prefixed with `who`.
SLICER_FFT_INTERNAL int slicer_fft_create(slicer_handle h, int npix, int split, hipStream_t st, int device,
                                          const char *who, slicer_fft_s **out);
SLICER_FFT_INTERNAL void slicer_fft_destroy(slicer_fft_s *f);

// The real npix^2 map a forward transform takes, formed as its rows are loaded and never stored: the f32 map x; the f32
// products x * y (one rounding); the f64 products x * y of two f64 maps; sqrt(x * x + y * y) of two f64 maps, rounded
// after every operation.
enum { FFT_ROWS_F32 = 0, FFT_ROWS_MASKED, FFT_ROWS_PRODUCT, FFT_ROWS_HYPOT };
struct FftRows {
    int kind;
    const void *x, *y;
};
// khat = rfft2(src) in f64, [npix][npix/2+1] (re, im) pairs.
SLICER_FFT_INTERNAL int slicer_fft_r2c(slicer_fft_s *f, hipStream_t st, const FftRows &src, double2 *khat);

// The half-plane spectrum an inverse transform takes, formed as its columns are loaded: khat times the shear filter
// `which` (SLICER_SHEAR_PHI .. _GAMMA2 with phi_c = -2 / (2 pi / theta)^2, _ALPHA1 / _ALPHA2 with alpha_c =
// -2 / (2 pi / theta)), 0 at k = 0; khat (NULL: ones) inside a band, 0 outside; |khat|^2.  A mode is in the band iff
// lo2 <= m2 < hi2 on the exact integer m2 (m2 <= hi2 with closed != 0) and m2 != 0 (with keep_dc != 0, m2 = 0 is in the
// band like any other mode).
enum { FFT_COLS_FILTER = 0, FFT_COLS_BAND, FFT_COLS_ABS2 };
struct FftCols {
    int kind;
    const double2 *khat;
    int which;
    double phi_c, alpha_c;
    double lo2, hi2;
    int closed, keep_dc;
};
// Where an inverse transform leaves its npix^2 values, each times 1 / npix^2: the f32 map out (rounded once); the f64
// map out; out as npix * (npix/2+1) complex f64 that only FFT_SINK_GAMMA reads, not yet scaled; or, with gamma1 left so
// in `packed` and this transform being gamma2's, the f32 maps out = gamma1, out2 = gamma2 and out3 = |gamma|.
enum { FFT_SINK_F32 = 0, FFT_SINK_F64, FFT_SINK_PACKED, FFT_SINK_GAMMA };
struct FftSink {
    int kind;
    void *out;
    float *out2, *out3;
    const double2 *packed;
};
// dst = irfft2(src), s = (npix, npix), in f64.
SLICER_FFT_INTERNAL int slicer_fft_c2r(slicer_fft_s *f, hipStream_t st, const FftCols &src, const FftSink &dst);

inline int slicer_fft_forward(slicer_fft_s *f, hipStream_t st, const float *map, double2 *khat)
{
    return slicer_fft_r2c(f, st, FftRows{FFT_ROWS_F32, map, nullptr}, khat);
}
// khat = rfft2(mask * map), the products taken in f32 (one rounding) as the rows are loaded: bitwise
// slicer_fft_forward of the multiplied map.
inline int slicer_fft_forward_masked(slicer_fft_s *f, hipStream_t st, const float *map, const float *mask, double2 *khat)
{
    return slicer_fft_r2c(f, st, FftRows{FFT_ROWS_MASKED, map, mask}, khat);
}
// khat = rfft2(x * y) for two f64 npix^2 maps, the products taken in f64 as the rows are loaded.
inline int slicer_fft_forward_product(slicer_fft_s *f, hipStream_t st, const double *x, const double *y, double2 *khat)
{
    return slicer_fft_r2c(f, st, FftRows{FFT_ROWS_PRODUCT, x, y}, khat);
}
// khat = rfft2(sqrt(x * x + y * y)) for two f64 npix^2 maps; the modulus is never stored.
inline int slicer_fft_forward_hypot(slicer_fft_s *f, hipStream_t st, const double *x, const double *y, double2 *khat)
{
    return slicer_fft_r2c(f, st, FftRows{FFT_ROWS_HYPOT, x, y}, khat);
}
// out = irfft2(khat * 1[mode in band]), kept in f64: npix^2 doubles.  khat = NULL: the transform of the band's
// indicator itself.
inline int slicer_fft_inverse_band(slicer_fft_s *f, hipStream_t st, const double2 *khat, double lo2, double hi2,
                                   int closed, double *out, int keep_dc = 0)
{
    return slicer_fft_c2r(f, st, FftCols{FFT_COLS_BAND, khat, 0, 0.0, 0.0, lo2, hi2, closed, keep_dc},
                          FftSink{FFT_SINK_F64, out});
}
// out = irfft2(|khat|^2), kept in f64: npix^2 doubles.
inline int slicer_fft_inverse_abs2(slicer_fft_s *f, hipStream_t st, const double2 *khat, double *out)
{
    return slicer_fft_c2r(f, st, FftCols{FFT_COLS_ABS2, khat}, FftSink{FFT_SINK_F64, out});
}
