// slicer_fd.hip -- finite-difference deflection, convergence and shear of a lensing-potential map.
//
// The real-space mode of the reference's Lens/smr.py (derivative="gradient": gradientO4 and laplacian_O3 of
// Lens/derivatives.py), for maps that are not periodic.  On a line f of n >= 5 samples of spacing d:
//   D1 f[i] = (f[i-2] - 8 f[i-1] + 8 f[i+1] - f[i+2]) / (12 d)                  2 <= i <= n-3
//             (f[i+1] - f[i]) / d  for i = 0, 1;   (f[i] - f[i-1]) / d  for i = n-2, n-1
//   D2 f[i] = (-f[i-2] + 16 f[i-1] - 30 f[i] + 16 f[i+1] - f[i+2]) / (12 d^2)    2 <= i <= n-3
//             (2 f[i] - 5 f[i+-1] + 4 f[i+-2] - f[i+-3]) / d^2                   towards the inside at the four edge samples
// and from the f32 map phi (axis 0 slow, axis 1 contiguous):
//   a1 = D1_0 phi, a2 = D1_1 phi, p11 = D2_0 phi, p22 = D2_1 phi, p12 = D1_1 D1_0 phi (= D1_0 D1_1 phi: the two act on
//   different axes), kappa = (p11 + p22) / 2, gamma1 = (p11 - p22) / 2, gamma2 = p12, |gamma| = sqrt(gamma1^2 + gamma2^2)
// in f64 from the f32 samples, each output rounded once to f32.
//
// One kernel, k_fd.  A workgroup of 256 threads takes a tile of kT0 x kT1 = 16 x 64 pixels, stages it with a halo of two
// pixels in LDS as f32 (20 x 68 floats; the f32 values are exact, they are widened where they are used) and every thread
// computes four adjacent pixels of one row.  Every stencil above reaches at most two samples from its pixel -- the 5 x 5
// footprint of p12 included -- except the one-sided D2, which reaches three: near the low edge those are rows / columns
// 0 ... 4 of the first tile, which holds them; near the high edge a last tile of fewer than three rows or columns does
// not, and takes what its window lacks from the map itself (sample()).  Every quotient is one f64 division of an
// integer-weighted sum: sums of small integers times exactly representable samples stay exact, so polynomial maps are
// differentiated without any rounding (tests).  No atomics, nothing handed between workgroups: bitwise repeatable.
// Stores: a float4 per thread and output when every output pointer is on the 16-byte grid and npix is a multiple of 4
// (k_fd<true>), four floats otherwise (k_fd<false>); the values are the same.
//
// f64 roundings on the longest path, counted from the code below (no FMA contraction: -ffp-contract=off):
//   D1: numerator 2 (a difference, the sum), denominator 12 d 1, division 1                                   = 4
//   D2: numerator 3 (a sum of two samples, the difference of the pairs, minus 30 f), 12 (d d) 2, division 1   = 6
//   kappa, gamma1: D2 and one sum (the halving is exact)                                                      = 7
//   p12 = gamma2: numerator 2 + 2 (D1 numerator of D1 numerators), denominators 1 + 1 and their product 1,
//        division 1                                                                                           = 8
//   |gamma|: two squares and their sum (2 on the longest path), the square root 1, on top of gamma1 and gamma2
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "slicer_host.hpp"

namespace {

constexpr int kT0 = 16, kT1 = 64;  // tile: rows x columns
constexpr int kHalo = 2;
constexpr int kRows = kT0 + 2 * kHalo, kPitch = kT1 + 2 * kHalo;
constexpr int kPer = 4;            // adjacent pixels of a thread
constexpr int kThreads = kT0 * kT1 / kPer;
constexpr int kMaxN = 1 << 19;  // grid.y = npix / kT0 stays below 65536

struct FdArgs {
    const float *phi;
    float *out[SLICER_FD_COUNT];
    int n;
    double d, den1, dd, den2;  // spacing, 12 d, d d, 12 (d d)
};

// -1, 0, 1: sample i of a line of n takes the forward, the centred, the backward formula
__device__ inline int side(int i, int n) { return i < 2 ? -1 : (i > n - 3 ? 1 : 0); }

// numerators of D1 and D2 at sample i (s = side(i, n)); f(k) is sample k of the line
template <class F>
__device__ inline double d1_num(F f, int i, int s)
{
    if (s == 0)
        return (f(i - 2) - f(i + 2)) + 8.0 * (f(i + 1) - f(i - 1));
    return s < 0 ? f(i + 1) - f(i) : f(i) - f(i - 1);
}
template <class F>
__device__ inline double d2_num(F f, int i, int s)
{
    if (s == 0)
        return (16.0 * (f(i - 1) + f(i + 1)) - (f(i - 2) + f(i + 2))) - 30.0 * f(i);
    return (2.0 * f(i) - 5.0 * f(i - s)) + (4.0 * f(i - 2 * s) - f(i - 3 * s));
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_fd(FdArgs a)
{
    __shared__ float tile[kRows * kPitch];
    const int n = a.n;
    const int r0 = (int)blockIdx.y * kT0 - kHalo, c0 = (int)blockIdx.x * kT1 - kHalo;  // map index of tile[0]
    for (int t = threadIdx.x; t < kRows * kPitch; t += kThreads) {
        const int r = r0 + t / kPitch, c = c0 + t % kPitch;
        tile[t] = r >= 0 && r < n && c >= 0 && c < n ? a.phi[(size_t)r * n + c] : 0.0f;
    }
    __syncthreads();
    const int i = r0 + kHalo + (int)threadIdx.x / (kT1 / kPer), j0 = c0 + kHalo + (int)threadIdx.x % (kT1 / kPer) * kPer;
    if (i >= n || j0 >= n)
        return;
    // pixel (r, c) of the map: within two of a pixel of this tile, so in the window
    auto win = [&](int r, int c) { return (double)tile[(r - r0) * kPitch + (c - c0)]; };
    // the same up to three away (one-sided D2): from the map where the window ends
    auto sample = [&](int r, int c) {
        const int lr = r - r0, lc = c - c0;
        if (lr >= 0 && lr < kRows && lc >= 0 && lc < kPitch)
            return (double)tile[lr * kPitch + lc];
        return (double)a.phi[(size_t)r * n + c];
    };
    const bool want_a1 = a.out[SLICER_FD_ALPHA1], want_a2 = a.out[SLICER_FD_ALPHA2];
    const bool want_k = a.out[SLICER_FD_KAPPA], want_g1 = a.out[SLICER_FD_GAMMA1], want_g2 = a.out[SLICER_FD_GAMMA2];
    const bool want_g = a.out[SLICER_FD_GAMMA];
    const int si = side(i, n);
    const double di = si ? a.d : a.den1, ddi = si ? a.dd : a.den2;
    float v[SLICER_FD_COUNT][kPer] = {};
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        const int j = j0 + q;
        if (j >= n)
            break;
        const int sj = side(j, n);
        const double dj = sj ? a.d : a.den1, ddj = sj ? a.dd : a.den2;
        if (want_a1)
            v[SLICER_FD_ALPHA1][q] = (float)(d1_num([&](int k) { return win(k, j); }, i, si) / di);
        if (want_a2)
            v[SLICER_FD_ALPHA2][q] = (float)(d1_num([&](int k) { return win(i, k); }, j, sj) / dj);
        double g1 = 0.0, g2 = 0.0;
        if (want_k || want_g1 || want_g) {
            const double p11 = d2_num([&](int k) { return sample(k, j); }, i, si) / ddi;
            const double p22 = d2_num([&](int k) { return sample(i, k); }, j, sj) / ddj;
            g1 = 0.5 * (p11 - p22);
            if (want_k)
                v[SLICER_FD_KAPPA][q] = (float)(0.5 * (p11 + p22));
            if (want_g1)
                v[SLICER_FD_GAMMA1][q] = (float)g1;
        }
        if (want_g2 || want_g) {
            const double num = d1_num([&](int c) { return d1_num([&](int k) { return win(k, c); }, i, si); }, j, sj);
            g2 = num / (di * dj);
            if (want_g2)
                v[SLICER_FD_GAMMA2][q] = (float)g2;
        }
        if (want_g)
            v[SLICER_FD_GAMMA][q] = (float)sqrt(g1 * g1 + g2 * g2);
    }
    const size_t at = (size_t)i * n + j0;
#pragma unroll
    for (int o = 0; o < SLICER_FD_COUNT; o++) {
        if (!a.out[o])
            continue;
        if (VEC && j0 + kPer <= n) {
            *reinterpret_cast<float4 *>(a.out[o] + at) = make_float4(v[o][0], v[o][1], v[o][2], v[o][3]);
        } else {
#pragma unroll
            for (int q = 0; q < kPer; q++)
                if (j0 + q < n)
                    a.out[o][at + q] = v[o][q];
        }
    }
}

}  // namespace

int slicer_fd_derivatives(slicer_handle h, int32_t npix, double spacing, const float *d_phi,
                          float *const d_out[SLICER_FD_COUNT])
{
    if (!h)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_fd_derivatives: null handle");
    if (npix < 5 || npix > kMaxN)
        return fail(h, SLICER_ERR_ARG, "slicer_fd_derivatives: npix = %d, expected 5..%d (the one-sided stencils take five samples)",
                    npix, kMaxN);
    if (!std::isfinite(spacing) || spacing <= 0.0)
        return fail(h, SLICER_ERR_ARG, "slicer_fd_derivatives: the spacing must be positive and finite");
    if (!d_phi || !d_out)
        return fail(h, SLICER_ERR_ARG, "slicer_fd_derivatives: null argument");
    FdArgs a{};
    a.phi = d_phi;
    a.n = npix;
    a.d = spacing;
    a.den1 = 12.0 * spacing;
    a.dd = spacing * spacing;
    a.den2 = 12.0 * a.dd;
    bool any = false, vec = npix % 4 == 0;
    for (int o = 0; o < SLICER_FD_COUNT; o++) {
        a.out[o] = d_out[o];
        if (!d_out[o])
            continue;
        if (d_out[o] == d_phi)
            return fail(h, SLICER_ERR_ARG, "slicer_fd_derivatives: output %d is the input map", o);
        any = true;
        vec = vec && (uintptr_t)d_out[o] % 16 == 0;
    }
    if (!any)
        return fail(h, SLICER_ERR_ARG, "slicer_fd_derivatives: every output is null");
    hipStream_t st;
    if (int rc = sub_stream(h, h->device, &st))
        return rc;
    const dim3 grid((unsigned)((npix + kT1 - 1) / kT1), (unsigned)((npix + kT0 - 1) / kT0));
    if (vec)
        hipLaunchKernelGGL(k_fd<true>, grid, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_fd<false>, grid, dim3(kThreads), 0, st, a);
    HIPCHK(h, hipGetLastError());
    return SLICER_OK;
}
