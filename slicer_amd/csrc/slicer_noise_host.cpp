// slicer_noise_host.cpp -- the host side of the shape noise: the generator's words, the noise of
// a pixel from a survey's numbers, and the gain of the smoothing filters of row N12 on white noise.  No device needed.
#include <cmath>
#include <vector>

#include "slicer_host.hpp"
#include "slicer_philox.hpp"

extern "C" {

int slicer_noise_words(uint64_t seed, uint32_t stream, uint32_t realisation, uint64_t block, uint32_t out[4])
{
    if (!out)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_noise_words: null argument");
    uint32_t w[4];
    slicer::noise_block_words(seed, stream, realisation, block, w);
    for (int k = 0; k < 4; k++)
        out[k] = w[k];
    return SLICER_OK;
}

int slicer_noise_sigma_pix(double sigma_e, double ngal_arcmin2, double angle_deg, int32_t npix, double *sigma_pix)
{
    const char *who = "slicer_noise_sigma_pix";
    if (!std::isfinite(sigma_e) || !(sigma_e > 0))
        return fail(nullptr, SLICER_ERR_ARG, "%s: sigma_e must be positive and finite", who);
    if (!std::isfinite(ngal_arcmin2) || !(ngal_arcmin2 > 0))
        return fail(nullptr, SLICER_ERR_ARG, "%s: the galaxy density must be positive and finite", who);
    if (!std::isfinite(angle_deg) || !(angle_deg > 0))
        return fail(nullptr, SLICER_ERR_ARG, "%s: the angle must be positive and finite", who);
    if (npix < 1)
        return fail(nullptr, SLICER_ERR_ARG, "%s: npix must be positive", who);
    if (!sigma_pix)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    const double side = 60.0 * angle_deg / (double)npix;  // of a pixel, arcminutes
    const double s = sigma_e / std::sqrt(ngal_arcmin2 * (side * side));
    if (!std::isfinite(s) || !(s > 0))
        return fail(nullptr, SLICER_ERR_ARG, "%s: the result is not a positive, finite number", who);
    *sigma_pix = s;
    return SLICER_OK;
}

int slicer_smooth_noise_gain(int32_t kind, double sigma_pix, double truncate, double *gain)
{
    const char *who = "slicer_smooth_noise_gain";
    if (kind != SLICER_SMOOTH_GAUSS && kind != SLICER_SMOOTH_MAP)
        return fail(nullptr, SLICER_ERR_ARG, "%s: kind = %d is neither SLICER_SMOOTH_GAUSS nor SLICER_SMOOTH_MAP", who, kind);
    int32_t R = 0;
    if (int rc = slicer_smooth_weights(sigma_pix, truncate, &R, nullptr, nullptr))
        return rc;
    if (!gain)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    std::vector<double> g(R + 1), h(R + 1);
    if (int rc = slicer_smooth_weights(sigma_pix, truncate, nullptr, g.data(), h.data()))
        return rc;
    // sums over k = -R ... R of g, g g, h h and g h, the small terms first
    long double sg = 0, gg = 0, hh = 0, gh = 0;
    for (int k = R; k >= 0; k--) {
        const long double m = k ? 2.0L : 1.0L, gk = g[k], hk = h[k];
        sg += m * gk;
        gg += m * gk * gk;
        hh += m * hk * hk;
        gh += m * gk * hk;
    }
    if (kind == SLICER_SMOOTH_GAUSS) {
        *gain = (double)(gg / (sg * sg));
    } else {
        // sum_ij (g_i g_j - h_i g_j - g_i h_j)^2 = A^2 + 2 A B - 4 A C + 2 C^2 with A = sum g g, B = sum h h, C = sum g h
        const long double sum = gg * gg + 2 * gg * hh - 4 * gg * gh + 2 * gh * gh;
        const long double c = 1.0L / (2.0L * 3.14159265358979323846264338327950288L * (long double)sigma_pix * (long double)sigma_pix);
        *gain = (double)(c * sqrtl(sum > 0 ? sum : 0.0L));
    }
    return SLICER_OK;
}

}  // extern "C"
