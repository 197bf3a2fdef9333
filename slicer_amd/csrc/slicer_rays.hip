// slicer_rays.hip -- on-device multi-plane ray tracing through the lens planes.
//
// One ray per pixel of an n x n grid (axis 0 slow = component 1, axis 1 contiguous = component 2, as in N6 / N8).  The
// state of a ray is 12 f64: position b = (b1, b2) and direction t = (t1, t2) in pixel units, centred (b = beta / d,
// h = (n - 1) / 2), and the 2 x 2 matrices A = d beta / d theta, T = d t / d theta.  Start: b = t = (i - h, j - h),
// A = T = I, last plane distance chi = 0.  Every operation below is one IEEE f64 operation, rounded once, in the order
// written (-ffp-contract=off: no FMA), so that a numpy restatement reproduces the device bit for bit.
//
// Step to the plane at chi_k > chi_{k-1}, described by five f32 maps (alpha1, alpha2 in radians, kappa, gamma1, gamma2),
// with w = (chi_k - chi_{k-1}) / chi_k from the host:
//   1. b_a += w (t_a - b_a);  A_ab += w (T_ab - A_ab)
//   2. u_a = b_a + h, i_a = floor(u_a), f_a = u_a - i_a, g_a = 1 - f_a; the cell's corners are i_a mod n and
//      (i_a + 1) mod n, the mathematical modulo (the grid wraps).  A ray whose u is not finite or has |u| >= 2^30 in
//      either component reads pixel (0, 0) with f = NaN: everything it computes from here on is NaN.
//   3. per map, samples widened exactly to f64: r0 = g2 m00 + f2 m01, r1 = g2 m10 + f2 m11, v = g1 r0 + f1 r1
//   4. U11 = v_kappa + v_gamma1, U22 = v_kappa - v_gamma1, U12 = U21 = v_gamma2
//   5. t_a -= v_alpha_a / d
//   6. T_ab -= U_a1 A_1b + U_a2 A_2b          (the A of step 1)
// Observe at chi_s >= chi of the last plane, w_s = (chi_s - chi) / chi_s: bs, As from step 1 with w_s (the state is not
// written), then, each formed in f64 and rounded once to f32,
//   kappa = 1 - 0.5 (As11 + As22), gamma1 = 0.5 (As22 - As11), gamma2 = -0.5 (As12 + As21), omega = 0.5 (As21 - As12),
//   delta_a = (theta_a - bs_a) d,   theta = (i - h, j - h) from the pixel index.
//
// k_rays_step<FIRST, VEC>: the state is twelve separate f64 arrays of n^2, updated in place (a thread reads and writes
// only its own rays).  A workgroup of 256 threads covers a tile of kT0 x kT1 = 8 x 64 rays, a thread two adjacent rays of
// a row: a wave reads and writes two whole 512-byte row segments of every state array, as double2 when n is even (VEC;
// the arrays are the library's own allocations, 16-byte aligned, and i n + j0 is then even), as scalars otherwise, with
// the same mapping and the same bits.  The tile is compact in both directions, so neighbouring rays, which land on
// neighbouring pixels unless the deflections scatter them, gather their f32 samples from few cache lines; the gathers are
// plain global loads, there is no LDS and there are no atomics.  FIRST builds the start state from the pixel index
// instead of reading it: neither create nor reset launches anything, and the first plane reads no state.
// k_rays_observe<FIRST, VEC>: the same mapping; reads the state arrays behind the outputs that were asked for (b_a and
// t_a for delta_a; the diagonals of A and T for kappa and gamma1, the off-diagonals for gamma2 and omega: all twelve
// for all six) and writes those outputs, two adjacent floats of a thread as a float2 when n is even and every output is
// on the 8-byte grid.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_host.hpp"

namespace {

constexpr int kT0 = 8, kT1 = 64;  // tile: rows x columns
constexpr int kPer = 2;           // adjacent rays of a thread
constexpr int kThreads = kT0 * kT1 / kPer;
constexpr int kMaxNpix = 131072;  // grid.y = npix / kT0 stays below 65536
constexpr int kState = 12;
// order of the state arrays (slicer_rays_state)
enum { B1 = 0, B2, T1, T2, A11, A12, A21, A22, T11, T12, T21, T22 };
enum { M_ALPHA1 = 0, M_ALPHA2, M_KAPPA, M_GAMMA1, M_GAMMA2, M_COUNT };

static_assert(kThreads == 256, "one thread per two rays of a tile");

struct StepArgs {
    double *s[kState];
    const float *m[M_COUNT];
    int n;
    double w, d, h;
};

struct ObserveArgs {
    const double *s[kState];
    float *out[SLICER_RAYS_COUNT];
    int n;
    double w, d, h;
};

template <bool VEC>
__device__ inline void load2(const double *p, size_t at, bool two, double &x, double &y)
{
    if (VEC) {
        const double2 v = *reinterpret_cast<const double2 *>(p + at);
        x = v.x, y = v.y;
    } else {
        x = p[at];
        y = two ? p[at + 1] : 0.0;
    }
}

template <bool VEC>
__device__ inline void store2(double *p, size_t at, bool two, double x, double y)
{
    if (VEC) {
        *reinterpret_cast<double2 *>(p + at) = make_double2(x, y);
    } else {
        p[at] = x;
        if (two)
            p[at + 1] = y;
    }
}

// the start state of the ray of pixel (i, j)
__device__ inline void start_state(double s[kState], int i, int j, double h)
{
    s[B1] = s[T1] = (double)i - h;
    s[B2] = s[T2] = (double)j - h;
    s[A11] = s[A22] = s[T11] = s[T22] = 1.0;
    s[A12] = s[A21] = s[T12] = s[T21] = 0.0;
}

// step 1: x + w (y - x)
__device__ inline double advance(double x, double y, double w) { return x + w * (y - x); }

// i mod n and (i + 1) mod n into 0 ... n-1, |i| <= 2^30
__device__ inline void wrap(int i, int n, int &lo, int &hi)
{
    lo = i % n;
    if (lo < 0)
        lo += n;
    hi = lo + 1 == n ? 0 : lo + 1;
}

template <bool FIRST, bool VEC>
__global__ __launch_bounds__(kThreads) void k_rays_step(StepArgs a)
{
    const int n = a.n;
    const int i = (int)blockIdx.y * kT0 + (int)threadIdx.x / (kT1 / kPer);
    const int j0 = (int)blockIdx.x * kT1 + (int)threadIdx.x % (kT1 / kPer) * kPer;
    if (i >= n || j0 >= n)
        return;
    const bool two = j0 + 1 < n;  // (always with VEC: n is even and so is j0)
    const size_t at = (size_t)i * n + j0;
    double s[kPer][kState];
    if (FIRST) {
#pragma unroll
        for (int q = 0; q < kPer; q++)
            start_state(s[q], i, j0 + q, a.h);
    } else {
#pragma unroll
        for (int k = 0; k < kState; k++)
            load2<VEC>(a.s[k], at, two, s[0][k], s[1][k]);
    }
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        if (q == 1 && !two)
            break;
        double *r = s[q];
        r[B1] = advance(r[B1], r[T1], a.w);
        r[B2] = advance(r[B2], r[T2], a.w);
        r[A11] = advance(r[A11], r[T11], a.w);
        r[A12] = advance(r[A12], r[T12], a.w);
        r[A21] = advance(r[A21], r[T21], a.w);
        r[A22] = advance(r[A22], r[T22], a.w);
        const double u1 = r[B1] + a.h, u2 = r[B2] + a.h;
        const bool ok = fabs(u1) < 0x1p30 && fabs(u2) < 0x1p30;  // false for NaN and the infinities too
        const double fl1 = floor(u1), fl2 = floor(u2);
        int lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0;
        double f1 = __builtin_nan(""), f2 = __builtin_nan("");
        if (ok) {
            wrap((int)fl1, n, lo1, hi1);
            wrap((int)fl2, n, lo2, hi2);
            f1 = u1 - fl1;
            f2 = u2 - fl2;
        }
        const double g1 = 1.0 - f1, g2 = 1.0 - f2;
        const size_t o00 = (size_t)lo1 * n + lo2, o01 = (size_t)lo1 * n + hi2;
        const size_t o10 = (size_t)hi1 * n + lo2, o11 = (size_t)hi1 * n + hi2;
        double v[M_COUNT];
#pragma unroll
        for (int m = 0; m < M_COUNT; m++) {
            const double m00 = (double)a.m[m][o00], m01 = (double)a.m[m][o01];
            const double m10 = (double)a.m[m][o10], m11 = (double)a.m[m][o11];
            const double r0 = g2 * m00 + f2 * m01;
            const double r1 = g2 * m10 + f2 * m11;
            v[m] = g1 * r0 + f1 * r1;
        }
        const double U11 = v[M_KAPPA] + v[M_GAMMA1], U22 = v[M_KAPPA] - v[M_GAMMA1], U12 = v[M_GAMMA2];
        r[T1] = r[T1] - v[M_ALPHA1] / a.d;
        r[T2] = r[T2] - v[M_ALPHA2] / a.d;
        r[T11] = r[T11] - (U11 * r[A11] + U12 * r[A21]);
        r[T12] = r[T12] - (U11 * r[A12] + U12 * r[A22]);
        r[T21] = r[T21] - (U12 * r[A11] + U22 * r[A21]);
        r[T22] = r[T22] - (U12 * r[A12] + U22 * r[A22]);
    }
#pragma unroll
    for (int k = 0; k < kState; k++)
        store2<VEC>(a.s[k], at, two, s[0][k], s[1][k]);
}

template <bool FIRST, bool VEC>
__global__ __launch_bounds__(kThreads) void k_rays_observe(ObserveArgs a)
{
    const int n = a.n;
    const int i = (int)blockIdx.y * kT0 + (int)threadIdx.x / (kT1 / kPer);
    const int j0 = (int)blockIdx.x * kT1 + (int)threadIdx.x % (kT1 / kPer) * kPer;
    if (i >= n || j0 >= n)
        return;
    const bool two = j0 + 1 < n;
    const size_t at = (size_t)i * n + j0;
    double s[kPer][kState] = {};
    if (FIRST) {
#pragma unroll
        for (int q = 0; q < kPer; q++)
            start_state(s[q], i, j0 + q, a.h);
    } else {
        // only the arrays behind the outputs that were asked for (the same in every thread)
        const bool diag = a.out[SLICER_RAYS_KAPPA] || a.out[SLICER_RAYS_GAMMA1];
        const bool off = a.out[SLICER_RAYS_GAMMA2] || a.out[SLICER_RAYS_OMEGA];
        const bool p1 = a.out[SLICER_RAYS_DEFLECTION1], p2 = a.out[SLICER_RAYS_DEFLECTION2];
        const bool need[kState] = {p1, p2, p1, p2, diag, off, off, diag, diag, off, off, diag};
#pragma unroll
        for (int k = 0; k < kState; k++)
            if (need[k])
                load2<VEC>(a.s[k], at, two, s[0][k], s[1][k]);
    }
    float o[SLICER_RAYS_COUNT][kPer] = {};
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        if (q == 1 && !two)
            break;
        const double *r = s[q];
        const double b1 = advance(r[B1], r[T1], a.w), b2 = advance(r[B2], r[T2], a.w);
        const double a11 = advance(r[A11], r[T11], a.w), a12 = advance(r[A12], r[T12], a.w);
        const double a21 = advance(r[A21], r[T21], a.w), a22 = advance(r[A22], r[T22], a.w);
        const double th1 = (double)i - a.h, th2 = (double)(j0 + q) - a.h;
        o[SLICER_RAYS_KAPPA][q] = (float)(1.0 - 0.5 * (a11 + a22));
        o[SLICER_RAYS_GAMMA1][q] = (float)(0.5 * (a22 - a11));
        o[SLICER_RAYS_GAMMA2][q] = (float)(-0.5 * (a12 + a21));
        o[SLICER_RAYS_OMEGA][q] = (float)(0.5 * (a21 - a12));
        o[SLICER_RAYS_DEFLECTION1][q] = (float)((th1 - b1) * a.d);
        o[SLICER_RAYS_DEFLECTION2][q] = (float)((th2 - b2) * a.d);
    }
#pragma unroll
    for (int k = 0; k < SLICER_RAYS_COUNT; k++) {
        if (!a.out[k])
            continue;
        if (VEC) {
            *reinterpret_cast<float2 *>(a.out[k] + at) = make_float2(o[k][0], o[k][1]);
        } else {
            a.out[k][at] = o[k][0];
            if (two)
                a.out[k][at + 1] = o[k][1];
        }
    }
}

dim3 rays_grid(int n) { return dim3((unsigned)((n + kT1 - 1) / kT1), (unsigned)((n + kT0 - 1) / kT0)); }

bool positive_finite(double x) { return std::isfinite(x) && x > 0.0; }

}  // namespace

struct slicer_rays : SubHandle {
    int n = 0;
    double d = 0.0;
    double *s[kState] = {};
    int n_steps = 0;
    double chi_last = 0.0;
};

extern "C" {

int slicer_rays_create(slicer_handle h, int32_t npix, double spacing, slicer_rays_handle *out)
{
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    const char *who = "slicer_rays_create";
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, who, npix, kMaxNpix))
        return rc;
    if (!positive_finite(spacing))
        return fail(h, SLICER_ERR_ARG, "slicer_rays_create: the spacing must be positive and finite");
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_rays_create: null argument");
    hipStream_t st = nullptr;
    slicer_rays_handle rh = nullptr;
    if (int rc = sub_new(h, who, &st, &rh))
        return rc;
    rh->n = npix;
    rh->d = spacing;
    int rc = SLICER_OK;
    for (int k = 0; k < kState; k++)
        rc = rh->mem.alloc(rc, h, who, (void **)&rh->s[k], (size_t)npix * (size_t)npix * sizeof(double));
    return sub_done(rc, rh, out);
}

int slicer_rays_reset(slicer_rays_handle rh)
{
    if (!rh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_rays_reset: null handle");
    rh->n_steps = 0;
    rh->chi_last = 0.0;
    return SLICER_OK;
}

int slicer_rays_step(slicer_rays_handle rh, double chi, const float *d_alpha1, const float *d_alpha2,
                     const float *d_kappa, const float *d_gamma1, const float *d_gamma2)
{
    slicer_handle h = rh ? rh->h : nullptr;
    if (!std::isfinite(chi))
        return fail(h, SLICER_ERR_ARG, "slicer_rays_step: chi must be finite");
    if (!d_alpha1 || !d_alpha2 || !d_kappa || !d_gamma1 || !d_gamma2)
        return fail(h, SLICER_ERR_ARG, "slicer_rays_step: null map");
    if (!rh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_rays_step: null handle");
    if (!(chi > rh->chi_last))
        return fail(h, SLICER_ERR_ARG, "slicer_rays_step: chi = %.17g is not above the last plane's %.17g", chi, rh->chi_last);
    hipStream_t st;
    if (int rc = sub_stream(h, rh->device, &st))
        return rc;
    StepArgs a{};
    for (int k = 0; k < kState; k++)
        a.s[k] = rh->s[k];
    a.m[M_ALPHA1] = d_alpha1, a.m[M_ALPHA2] = d_alpha2;
    a.m[M_KAPPA] = d_kappa, a.m[M_GAMMA1] = d_gamma1, a.m[M_GAMMA2] = d_gamma2;
    a.n = rh->n;
    a.w = (chi - rh->chi_last) / chi;
    a.d = rh->d;
    a.h = (double)(rh->n - 1) / 2.0;
    const bool first = rh->n_steps == 0, vec = rh->n % 2 == 0;
    {
        ProfScope ps(h, KN_RAYS_STEP);
        const dim3 grid = rays_grid(rh->n), block(kThreads);
        if (first && vec)
            hipLaunchKernelGGL((k_rays_step<true, true>), grid, block, 0, st, a);
        else if (first)
            hipLaunchKernelGGL((k_rays_step<true, false>), grid, block, 0, st, a);
        else if (vec)
            hipLaunchKernelGGL((k_rays_step<false, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_rays_step<false, false>), grid, block, 0, st, a);
        HIPCHK(h, hipGetLastError());
    }
    rh->n_steps++;
    rh->chi_last = chi;
    return SLICER_OK;
}

int slicer_rays_observe(slicer_rays_handle rh, double chi_s, float *const d_out[SLICER_RAYS_COUNT])
{
    slicer_handle h = rh ? rh->h : nullptr;
    if (!positive_finite(chi_s))
        return fail(h, SLICER_ERR_ARG, "slicer_rays_observe: chi_s must be positive and finite");
    if (!d_out)
        return fail(h, SLICER_ERR_ARG, "slicer_rays_observe: null argument");
    bool any = false, aligned = true;
    for (int k = 0; k < SLICER_RAYS_COUNT; k++) {
        any = any || d_out[k];
        aligned = aligned && (uintptr_t)d_out[k] % 8 == 0;
    }
    if (!any)
        return fail(h, SLICER_ERR_ARG, "slicer_rays_observe: every output is null");
    if (!rh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_rays_observe: null handle");
    if (chi_s < rh->chi_last)
        return fail(h, SLICER_ERR_ARG, "slicer_rays_observe: chi_s = %.17g is below the last plane's %.17g", chi_s,
                    rh->chi_last);
    hipStream_t st;
    if (int rc = sub_stream(h, rh->device, &st))
        return rc;
    ObserveArgs a{};
    for (int k = 0; k < kState; k++)
        a.s[k] = rh->s[k];
    for (int k = 0; k < SLICER_RAYS_COUNT; k++)
        a.out[k] = d_out[k];
    a.n = rh->n;
    a.w = (chi_s - rh->chi_last) / chi_s;
    a.d = rh->d;
    a.h = (double)(rh->n - 1) / 2.0;
    const bool first = rh->n_steps == 0, vec = rh->n % 2 == 0 && aligned;
    {
        ProfScope ps(h, KN_RAYS_OBSERVE);
        const dim3 grid = rays_grid(rh->n), block(kThreads);
        if (first && vec)
            hipLaunchKernelGGL((k_rays_observe<true, true>), grid, block, 0, st, a);
        else if (first)
            hipLaunchKernelGGL((k_rays_observe<true, false>), grid, block, 0, st, a);
        else if (vec)
            hipLaunchKernelGGL((k_rays_observe<false, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_rays_observe<false, false>), grid, block, 0, st, a);
        HIPCHK(h, hipGetLastError());
    }
    return SLICER_OK;
}

int slicer_rays_state(slicer_rays_handle rh, double *host)
{
    if (!rh || !host)
        return fail(rh ? rh->h : nullptr, SLICER_ERR_ARG, "slicer_rays_state: null argument");
    hipStream_t st;
    if (int rc = sub_stream(rh->h, rh->device, &st))
        return rc;
    const size_t n = (size_t)rh->n, n2 = n * n;
    if (rh->n_steps == 0) {  // the start state lives nowhere on the device: the first step builds it
        HIPCHK(rh->h, hipStreamSynchronize(st));
        const double hh = (double)(rh->n - 1) / 2.0;
        for (size_t i = 0; i < n; i++)
            for (size_t j = 0; j < n; j++) {
                const size_t at = i * n + j;
                host[B1 * n2 + at] = host[T1 * n2 + at] = (double)i - hh;
                host[B2 * n2 + at] = host[T2 * n2 + at] = (double)j - hh;
                host[A11 * n2 + at] = host[A22 * n2 + at] = host[T11 * n2 + at] = host[T22 * n2 + at] = 1.0;
                host[A12 * n2 + at] = host[A21 * n2 + at] = host[T12 * n2 + at] = host[T21 * n2 + at] = 0.0;
            }
        return SLICER_OK;
    }
    for (int k = 0; k < kState; k++)
        HIPCHK(rh->h, hipMemcpyAsync(host + k * n2, rh->s[k], n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(rh->h, hipStreamSynchronize(st));
    return SLICER_OK;
}

int slicer_rays_planes(slicer_rays_handle rh, int32_t *n_steps, double *chi_last)
{
    if (!rh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_rays_planes: null handle");
    if (n_steps)
        *n_steps = rh->n_steps;
    if (chi_last)
        *chi_last = rh->chi_last;
    return SLICER_OK;
}

int slicer_rays_destroy(slicer_rays_handle rh) { return sub_destroy(rh); }

}  // extern "C"
