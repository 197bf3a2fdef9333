// slicer_shear.hip -- on-device lensing potential and shear maps from a kappa map.
//
// With K0 = 2 pi fftfreq(n, d) along axis 0 (rows), K1 = 2 pi rfftfreq(n, d) along axis 1 (the contiguous axis),
// k^2 = K0^2 + K1^2, d = theta / n and every quotient 0 at k = 0:
//   khat = rfft2(kappa);  phi = irfft2(-2 khat / k^2);  gamma1 = irfft2(khat (K0^2 - K1^2) / k^2);
//   gamma2 = irfft2(khat 2 K0 K1 / k^2);  |gamma| = sqrt(gamma1^2 + gamma2^2)
// in f64, every output rounded once to f32: one forward transform and three inverses of slicer_fft.hip, which fuses
// the filters into its column loads.  gamma1's inverse leaves its rows in f64 (G); gamma2's reads them and writes
// gamma1, gamma2 and |gamma|.  The deflection maps (row N8, slicer_shear_deflection) are two more inverses of the kept
// spectrum: the filter cases alpha1 = i K0 phihat and alpha2 = i K1 phihat.  This file holds no kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "slicer_fft.hpp"
#include "slicer_host.hpp"

struct slicer_shear_s : SubHandle {
    slicer_fft_s *fft = nullptr;
    int n = 0;
    double angle = 0.0;
    double2 *S = nullptr, *G = nullptr;  // complex f64, n * H each
    float *maps[4] = {nullptr, nullptr, nullptr, nullptr};
    float *alpha[2] = {nullptr, nullptr};  // allocated by the first slicer_shear_deflection
    float *fd[SLICER_FD_COUNT] = {};       // allocated by the first slicer_shear_fd
    bool ran = false;
    bool alpha_ok = false, fd_ok = false;  // alpha / fd belong to the last run
    SLICER_FFT_INTERNAL ~slicer_shear_s() { slicer_fft_destroy(fft); }
};

int slicer_shear_supported(int32_t n) { return fft_size_supported(n) ? 1 : 0; }

int slicer_shear_create(slicer_handle h, int32_t npix, double angle_deg, slicer_shear_handle *out)
{
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_shear_create: null argument");
    *out = nullptr;
    if (!fft_size_supported(npix))
        return fail(h, SLICER_ERR_UNSUPPORTED,
                    "slicer_shear_create: npix = %d unsupported (2..%d, prime factors 2, 3, 5, 7 only)", npix, kFftMaxN);
    if (!std::isfinite(angle_deg) || angle_deg <= 0.0)
        return fail(h, SLICER_ERR_ARG, "slicer_shear_create: the angle must be positive and finite");
    const char *who = "slicer_shear_create";
    hipStream_t st = nullptr;
    slicer_shear_handle sh = nullptr;
    if (int rc = sub_new(h, who, &st, &sh))
        return rc;
    const int n = sh->n = npix;
    sh->angle = angle_deg;
    int rc = slicer_fft_create(h, n, h->opt.shear_split, st, sh->device, who, &sh->fft);
    const size_t cbytes = (size_t)n * (n / 2 + 1) * sizeof(double2);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->S, cbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->G, cbytes);
    for (float *&m : sh->maps)
        rc = sh->mem.alloc(rc, h, who, (void **)&m, (size_t)n * n * sizeof(float));
    return sub_done(rc, sh, out);
}

int slicer_shear_run(slicer_shear_handle sh, const float *d_kappa)
{
    if (!sh || !d_kappa)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_shear_run: null argument");
    hipStream_t st;
    if (int rc = sub_stream(sh->h, sh->device, &st))
        return rc;
    const double c = 2.0 * M_PI / (sh->angle * M_PI / 180.0);  // K = c * (fftfreq index)
    if (int rc = slicer_fft_forward(sh->fft, st, d_kappa, sh->S))
        return rc;
    // inverses of the filtered S -> maps (gamma1 -> G in f64 first; gamma2 also writes gamma1 and |gamma|)
    float **m = sh->maps;
    const FftSink sinks[] = {{FFT_SINK_F32, m[SLICER_SHEAR_PHI]}, {FFT_SINK_PACKED, sh->G},
                             {FFT_SINK_GAMMA, m[SLICER_SHEAR_GAMMA1], m[SLICER_SHEAR_GAMMA2], m[SLICER_SHEAR_GAMMA], sh->G}};
    for (int which : {SLICER_SHEAR_PHI, SLICER_SHEAR_GAMMA1, SLICER_SHEAR_GAMMA2})
        if (int rc = slicer_fft_c2r(sh->fft, st, FftCols{FFT_COLS_FILTER, sh->S, which, -2.0 / (c * c)}, sinks[which]))
            return rc;
    sh->ran = true;
    sh->alpha_ok = sh->fd_ok = false;
    return SLICER_OK;
}

int slicer_shear_deflection(slicer_shear_handle sh)
{
    if (!sh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_shear_deflection: null argument");
    if (!sh->ran)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_shear_deflection before any slicer_shear_run");
    hipStream_t st;
    if (int rc = sub_stream(sh->h, sh->device, &st))
        return rc;
    const int n = sh->n;
    int rc = SLICER_OK;
    for (float *&m : sh->alpha)
        if (!m)
            rc = sh->mem.alloc(rc, sh->h, "slicer_shear_deflection", (void **)&m, (size_t)n * n * sizeof(float));
    if (rc != SLICER_OK)
        return rc;
    sh->alpha_ok = false;
    const double alpha_c = -2.0 / (2.0 * M_PI / (sh->angle * M_PI / 180.0));
    // inverses of the filtered S -> maps, as for phi
    for (int a = 0; a < 2; a++)
        if (int r = slicer_fft_c2r(sh->fft, st, FftCols{FFT_COLS_FILTER, sh->S, SLICER_SHEAR_ALPHA1 + a, 0.0, alpha_c},
                                   FftSink{FFT_SINK_F32, sh->alpha[a]}))
            return r;
    sh->alpha_ok = true;
    return SLICER_OK;
}

int slicer_shear_fd(slicer_shear_handle sh)
{
    if (!sh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_shear_fd: null argument");
    const int n = sh->n;
    if (n < 5)
        return fail(sh->h, SLICER_ERR_UNSUPPORTED, "slicer_shear_fd: npix = %d, the stencils take at least 5", n);
    if (!sh->ran)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_shear_fd before any slicer_shear_run");
    hipStream_t st;
    if (int rc = sub_stream(sh->h, sh->device, &st))
        return rc;
    int rc = SLICER_OK;
    for (float *&m : sh->fd)
        if (!m)
            rc = sh->mem.alloc(rc, sh->h, "slicer_shear_fd", (void **)&m, (size_t)n * n * sizeof(float));
    if (rc != SLICER_OK)
        return rc;
    sh->fd_ok = false;
    if (int r = slicer_fd_derivatives(sh->h, n, sh->angle * M_PI / 180.0 / n, sh->maps[SLICER_SHEAR_PHI], sh->fd))
        return r;
    sh->fd_ok = true;
    return SLICER_OK;
}

int slicer_shear_spectrum(slicer_shear_handle sh, double *host)
{
    if (!sh || !host)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_shear_spectrum: null argument");
    if (!sh->ran)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_shear_spectrum before any slicer_shear_run");
    return sub_read(*sh, host, sh->S, (size_t)sh->n * (sh->n / 2 + 1) * sizeof(double2));
}

int slicer_shear_device_map(slicer_shear_handle sh, int32_t which, float **d_map)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_shear_device_map: null argument");
    if (which >= SLICER_SHEAR_PHI && which <= SLICER_SHEAR_GAMMA) {
        if (!sh->ran)
            return fail(sh->h, SLICER_ERR_STATE, "shear maps are available after slicer_shear_run");
        *d_map = sh->maps[which];
    } else if (which == SLICER_SHEAR_ALPHA1 || which == SLICER_SHEAR_ALPHA2) {
        if (!sh->alpha_ok)
            return fail(sh->h, SLICER_ERR_STATE,
                        "deflection maps are available after slicer_shear_deflection of the last slicer_shear_run");
        *d_map = sh->alpha[which - SLICER_SHEAR_ALPHA1];
    } else if (which >= SLICER_SHEAR_FD_ALPHA1 && which <= SLICER_SHEAR_FD_GAMMA) {
        if (!sh->fd_ok)
            return fail(sh->h, SLICER_ERR_STATE,
                        "finite-difference maps are available after slicer_shear_fd of the last slicer_shear_run");
        *d_map = sh->fd[which - SLICER_SHEAR_FD_ALPHA1];
    } else {
        return fail(sh->h, SLICER_ERR_ARG, "slicer_shear_device_map: which = %d, expected 0..3, 8, 9 or 16..21", which);
    }
    return SLICER_OK;
}

int slicer_shear_read(slicer_shear_handle sh, int32_t which, float *host)
{
    float *d = nullptr;
    if (int rc = slicer_shear_device_map(sh, which, &d))
        return rc;
    if (!host)
        return fail(sh->h, SLICER_ERR_ARG, "slicer_shear_read: null host pointer");
    return sub_read(*sh, host, d, (size_t)sh->n * sh->n * sizeof(float));
}

int slicer_shear_destroy(slicer_shear_handle sh) { return sub_destroy(sh); }
