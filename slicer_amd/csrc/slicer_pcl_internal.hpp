// slicer_pcl_internal.hpp -- internal (not exported): what the two pseudo-C_l handles share (slicer_pcl.hip, rows N17,
// and slicer_pcl_shear.hip, row N21): the mask and its moments, and the host f64 LU with partial pivoting behind the
// decoupling.
#pragma once

#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

#include "slicer_fft.hpp"
#include "slicer_host.hpp"

constexpr int kPclMomentGroups = 256;  // workgroups of the moments kernel: the partials the host adds up

// The mask of a set_mask after its argument checks, enqueued on st, errors under the name `who`: w [n^2] from the border
// taper of width taper_width_pix (0: none; d_f [n] holds its table) and the user mask d_mask (NULL: none), then mean(w)
// and mean(w^2) through d_partial and d_bad [kPclMomentGroups].  Waits for st.  A value of w that is not finite:
// SLICER_ERR_ARG.
SLICER_FFT_INTERNAL int pcl_build_mask(slicer_handle h, const char *who, hipStream_t st, int n, const float *d_mask,
                                       double taper_width_pix, float *d_w, double *d_f, double2 *d_partial,
                                       unsigned long long *d_bad, double *mean_w, double *mean_w2);

// LU with partial pivoting of the na x na matrix a (row-major, in place); false at a zero or non-finite pivot
inline bool lu_factor(std::vector<double> &a, int na, std::vector<int> &piv)
{
    piv.assign(na, 0);
    for (int k = 0; k < na; k++) {
        int p = k;
        double best = -1.0;
        for (int i = k; i < na; i++) {
            const double v = std::fabs(a[(size_t)i * na + k]);
            if (!std::isfinite(v))
                return false;
            if (v > best) {
                best = v;
                p = i;
            }
        }
        if (!(best > 0.0))
            return false;
        piv[k] = p;
        if (p != k)
            for (int j = 0; j < na; j++)
                std::swap(a[(size_t)k * na + j], a[(size_t)p * na + j]);
        const double d = a[(size_t)k * na + k];
        for (int i = k + 1; i < na; i++) {
            const double m = a[(size_t)i * na + k] / d;
            a[(size_t)i * na + k] = m;
            for (int j = k + 1; j < na; j++)
                a[(size_t)i * na + j] -= m * a[(size_t)k * na + j];
        }
    }
    for (double v : a)
        if (!std::isfinite(v))
            return false;
    return true;
}

// x <- (LU)^-1 P x: the row exchanges, the forward and the back substitution
inline void lu_solve(const std::vector<double> &a, int na, const std::vector<int> &piv, double *x)
{
    for (int k = 0; k < na; k++)
        std::swap(x[k], x[piv[k]]);
    for (int i = 1; i < na; i++) {
        double s = x[i];
        for (int j = 0; j < i; j++)
            s -= a[(size_t)i * na + j] * x[j];
        x[i] = s;
    }
    for (int i = na - 1; i >= 0; i--) {
        double s = x[i];
        for (int j = i + 1; j < na; j++)
            s -= a[(size_t)i * na + j] * x[j];
        x[i] = s / a[(size_t)i * na + i];
    }
}
