// slicer_scattering_filter.hpp -- internal: the Morlet filter of the scattering handle (the
// definition is in include/slicer_amd.h) as one f64 expression that slicer_scattering_filter (host) and k_scat_filter
// (device) both compile, so that the two differ by exp itself and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

struct ScatFilter {
    double h;       // sigma^2 / 2, sigma = 0.8 2^j
    double xi;      // (3 pi / 4) 2^-j
    double s2;      // s^2, s = 4 / L
    double ct, st;  // cos and sin of theta = pi l / L, from the host
    double beta;    // A^(0) / B^(0), from the host
};

constexpr double kScatTwoPi = 6.283185307179586476925286766559;

// the exponent of A (shift = xi) or B (shift = 0) at the angular frequency (w1, w2) along (axis 0, axis 1)
__host__ __device__ inline double scat_exponent(const ScatFilter &f, double w1, double w2, double shift)
{
    const double p = w1 * f.ct + w2 * f.st;
    const double q = -w1 * f.st + w2 * f.ct;
    const double d = p - shift;
    return -f.h * (d * d + q * q / f.s2);
}

// A^ and B^ at (w1, w2): the nine aliases, m1 outer, m2 inner, each from -1 up
__host__ __device__ inline void scat_alias_sums(const ScatFilter &f, double w1, double w2, double &A, double &B)
{
    A = 0.0;
    B = 0.0;
    for (int m1 = -1; m1 <= 1; m1++)
        for (int m2 = -1; m2 <= 1; m2++) {
            const double v1 = w1 + kScatTwoPi * (double)m1, v2 = w2 + kScatTwoPi * (double)m2;
            A = A + exp(scat_exponent(f, v1, v2, f.xi));
            B = B + exp(scat_exponent(f, v1, v2, 0.0));
        }
}

// psi^[a][b] of an n^2 map, 0 <= a, b < n
__host__ __device__ inline double scat_psi(const ScatFilter &f, int n, int a, int b)
{
    if (a == 0 && b == 0)
        return 0.0;
    const int as = a < (n + 1) / 2 ? a : a - n, bs = b < (n + 1) / 2 ? b : b - n;
    double A, B;
    scat_alias_sums(f, kScatTwoPi * (double)as / (double)n, kScatTwoPi * (double)bs / (double)n, A, B);
    return A - f.beta * B;
}
