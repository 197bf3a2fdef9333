// slicer_xi.hip -- on-device real-space two-point correlation functions of spin-0 and spin-2 maps under one shared weight
// map: xi_kk(theta), xi+(theta) and xi-(theta) (the definitions are in include/slicer_amd.h).
//
// The maps are not periodic: every n^2 map is zero-padded to P^2, P >= n + L a size the f64 transform plans, so that the
// circular correlation of the padded maps is the linear one at every lag |dx|, |dy| <= L.
// The transform is that of slicer_fft.hip; check_edges and first_at_least come from slicer_power_internal.hpp.
//   set_weights  k_xi_norm sums w^2 and counts the values that are negative or not finite; k_xi_pad writes w padded in
//                f64 (the second factor of every field load) and in f32; what = rfft2 (slicer_fft_forward), |what|^2
//                (k_xi_spectra), W(r) = irfft2 (slicer_fft_inverse_band, every mode kept), W_b and sum W sqrt(m2)
//                (k_xi_bin).  w = NULL: W(r) = N(r), and both sums come from the host's integers, no transform
//   run          per field component k_xi_pad to f64 and slicer_fft_forward_product with the padded weights: the exact
//                f64 products a * w, transformed; per pair and statistic k_xi_spectra, slicer_fft_inverse_band and k_xi_bin
//   read         sums / W_b on the host; NaN in the empty bins
// k_xi_bin: one workgroup per (kXiCols adjacent columns dy of the lag window, bin).  A thread owns one dy; the lags of
// the bin in that column are the run lo <= |dx| < hi (first_at_least, the rule of slicer_power.hip), walked upwards,
// +dx before -dx: the threads of a wave read adjacent doubles of one row.  The FULL window is walked, both signs of both
// lags, nothing is doubled.  A fixed wave butterfly gives one partial per (bin, column chunk); k_xi_sum adds a bin's
// partials in chunk order.  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_power_internal.hpp"
#include "slicer_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kXiCols = 64;       // columns (lags dy) of one k_xi_bin workgroup, one a thread: one wave
constexpr int kSumThreads = 256;  // sums of one k_xi_sum workgroup, one a thread
constexpr int kNormGroups = 256;  // workgroups of k_xi_norm: the partials the host adds up
constexpr int kMaxFields = 32;
constexpr int kMaxP = kFftMaxN;  // the largest padded size

enum { SPEC_0 = 0, SPEC_PLUS, SPEC_MINUS, SPEC_CROSS };  // k_xi_spectra
enum { BIN_PLAIN = 0, BIN_SPIN4, BIN_WEIGHT };           // k_xi_bin

// out[P][P] = in[n][n] (1 for NULL) in the corner at the origin, 0 elsewhere
template <class T>
__global__ __launch_bounds__(kThreads) void k_xi_pad(const float *in, T *out, int n, int P)
{
    const size_t total = (size_t)P * P;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int i0 = (int)(i / P), i1 = (int)(i - (size_t)i0 * P);
        T v = (T)0;
        if (i0 < n && i1 < n)
            v = in ? (T)in[(size_t)i0 * n + i1] : (T)1;
        out[i] = v;
    }
}

// partial[g] = the sum of w^2 over the good pixels i = g * 256 + t + k * 256 * groups, bad[g] = the number of the others
// (negative or not finite); every thread sums its pixels in index order, the workgroup in a fixed tree
__global__ __launch_bounds__(kThreads) void k_xi_norm(const float *w, size_t total, double *partial,
                                                      unsigned long long *bad)
{
    __shared__ double s2[kThreads];
    __shared__ unsigned long long sb[kThreads];
    double a = 0.0;
    unsigned long long nb = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const double v = (double)w[i];
        if (isfinite(v) && v >= 0.0)
            a += v * v;
        else
            nb++;
    }
    const int t = threadIdx.x;
    s2[t] = a;
    sb[t] = nb;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d /= 2) {
        if (t < d) {
            s2[t] += s2[t + d];
            sb[t] += sb[t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[blockIdx.x] = s2[0];
        bad[blockIdx.x] = sb[0];
    }
}

// out = (the real spectrum, 0) over the [P][P/2+1] half plane.  SPEC_0: Re(conj a1 b1); SPEC_PLUS: Re(conj a1 b1 +
// conj a2 b2); SPEC_MINUS: Re(conj a1 b1 - conj a2 b2); SPEC_CROSS: Re(conj a1 b2 + conj a2 b1).  out may be a1.
__global__ __launch_bounds__(kThreads) void k_xi_spectra(const double2 *a1, const double2 *a2, const double2 *b1,
                                                         const double2 *b2, double2 *out, size_t total, int mode)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        double v;
        if (mode == SPEC_0) {
            const double2 x = a1[i], y = b1[i];
            v = x.x * y.x + x.y * y.y;
        } else {
            const double2 x1 = a1[i], x2 = a2[i], y1 = b1[i], y2 = b2[i];
            if (mode == SPEC_CROSS)
                v = (x1.x * y2.x + x1.y * y2.y) + (x2.x * y1.x + x2.y * y1.y);
            else {
                const double p = x1.x * y1.x + x1.y * y1.y, q = x2.x * y2.x + x2.y * y2.y;
                v = mode == SPEC_PLUS ? p + q : p - q;
            }
        }
        out[i] = make_double2(v, 0.0);
    }
}

struct XiBinArgs {
    const double *r1, *r2;  // P^2 correlations; r2: BIN_SPIN4's second one
    const double *e2;       // edge squares, B + 1
    double *partial;        // [value][bin][chunk]; BIN_WEIGHT has two values, the others one
    int P, L, B, nchunks, mode;
};

// BIN_PLAIN: the sum of r1 over the bin's lags; BIN_SPIN4: of r1 c4 + r2 s4; BIN_WEIGHT: of r1 and of r1 sqrt(m2)
__global__ __launch_bounds__(kXiCols) void k_xi_bin(XiBinArgs a)
{
    const int tid = threadIdx.x, b = blockIdx.y, col = (int)blockIdx.x * kXiCols + tid, L = a.L, P = a.P;
    double acc0 = 0.0, acc1 = 0.0;
    if (col <= 2 * L) {
        const int dy = col - L;
        const double y = (double)dy, y2 = y * y;
        const size_t c = (size_t)(dy < 0 ? P + dy : dy);
        int lo = first_at_least(y2, a.e2[b], false, L + 1);
        const int hi = first_at_least(y2, a.e2[b + 1], b == a.B - 1, L + 1);
        if (dy == 0 && lo == 0)
            lo = 1;  // m2 = 0 is in no bin
        for (int ax = lo; ax < hi; ax++) {
            const double x = (double)ax, x2 = x * x, m2 = x2 + y2;
            double c4 = 0.0, s4 = 0.0, rad = 0.0;
            if (a.mode == BIN_SPIN4) {
                const double m4 = m2 * m2;
                c4 = (x2 * x2 - 6.0 * x2 * y2 + y2 * y2) / m4;
                s4 = 4.0 * x * y * (x2 - y2) / m4;  // of +dx; -dx flips its sign
            } else if (a.mode == BIN_WEIGHT) {
                rad = sqrt(m2);
            }
            for (int neg = 0; neg < (ax > 0 ? 2 : 1); neg++) {
                const size_t i = (size_t)(neg ? P - ax : ax) * P + c;
                const double v = a.r1[i];
                if (a.mode == BIN_SPIN4) {
                    acc0 += v * c4 + a.r2[i] * (neg ? -s4 : s4);
                } else {
                    acc0 += v;
                    acc1 += v * rad;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off /= 2) {
        acc0 += __shfl_xor(acc0, off, 64);
        acc1 += __shfl_xor(acc1, off, 64);
    }
    if (tid == 0) {
        a.partial[(size_t)b * a.nchunks + blockIdx.x] = acc0;
        if (a.mode == BIN_WEIGHT)
            a.partial[((size_t)a.B + b) * a.nchunks + blockIdx.x] = acc1;
    }
}

// out[i] = the sum of partial[i][0 .. nchunks-1] in chunk order
__global__ __launch_bounds__(kSumThreads) void k_xi_sum(const double *partial, int nchunks, int count, double *out)
{
    const int i = (int)blockIdx.x * kSumThreads + threadIdx.x;
    if (i >= count)
        return;
    double sum = 0.0;
    for (int k = 0; k < nchunks; k++)
        sum += partial[(size_t)i * nchunks + k];
    out[i] = sum;
}

// win[dx + L][dy + L] = r[dx mod P][dy mod P], |dx|, |dy| <= L
__global__ __launch_bounds__(kThreads) void k_xi_window(const double *r, double *win, int P, int L)
{
    const int W = 2 * L + 1;
    const size_t total = (size_t)W * W;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int dx = (int)(i / W) - L, dy = (int)(i % W) - L;
        win[i] = r[(size_t)(dx < 0 ? P + dx : dx) * P + (size_t)(dy < 0 ? P + dy : dy)];
    }
}

unsigned groups_for(size_t total) { return (unsigned)std::min<size_t>(4096, (total + kThreads - 1) / kThreads); }

// What the edges fix on the host.  Returns "" or why the edges cannot be used.
struct XiGeom {
    int n = 0, B = 0, L = 0, P = 0;  // P = 0: no supported size holds n + L
    std::vector<double> e2;
    std::vector<int64_t> counts, lags;  // N_b, M_b
    std::vector<double> nr;             // the sum of N(r) sqrt(m2) over the bin's lags
};

const char *xi_geom(int npix, int n_edges, const double *edges, XiGeom &g)
{
    if (!edges)
        return "the edges are required";
    std::vector<double> e;
    const char *why = check_edges(npix, n_edges, edges, e);
    if (*why)
        return why;
    const int n = npix, B = n_edges - 1;
    if (e[B] > std::sqrt(2.0) * (double)(n - 1))
        return "the last edge is beyond sqrt(2) (npix - 1)";
    g.n = n;
    g.B = B;
    g.L = (int)std::min((double)(n - 1), std::ceil(e[B]));
    g.P = 0;
    for (int p = n + g.L; p <= kMaxP && !g.P; p++)
        if (fft_size_supported(p))
            g.P = p;
    g.e2.resize(B + 1);
    for (int b = 0; b <= B; b++)
        g.e2[b] = e[b] * e[b];
    return "";
}

// N_b, M_b and the radius sums by enumeration of the quadrant dx, dy >= 0 (a lag off both axes stands for 4, on one for 2)
void xi_enumerate(XiGeom &g)
{
    const int B = g.B, L = g.L, n = g.n;
    g.counts.assign(B, 0);
    g.lags.assign(B, 0);
    std::vector<long double> sum(B, 0.0L);
    for (int dx = 0; dx <= L; dx++)
        for (int dy = dx ? 0 : 1; dy <= L; dy++) {
            const double m2 = (double)dx * dx + (double)dy * dy;
            int b = (int)(std::upper_bound(g.e2.begin(), g.e2.end(), m2) - g.e2.begin()) - 1;  // last edge <= m2
            if (b == B && m2 == g.e2[B])
                b = B - 1;
            if (b < 0 || b >= B)
                continue;
            const int64_t mult = (dx ? 2 : 1) * (dy ? 2 : 1), pairs = (int64_t)(n - dx) * (n - dy);
            g.lags[b] += mult;
            g.counts[b] += mult * pairs;
            sum[b] += (long double)(mult * pairs) * sqrtl((long double)m2);
        }
    g.nr.resize(B);
    for (int b = 0; b < B; b++)
        g.nr[b] = (double)sum[b];
}

}  // namespace

struct slicer_xi_s : SubHandle {
    slicer_fft_s *fft = nullptr;
    XiGeom g;
    int spin = 0, comps = 1, F = 0, cross = 0, npairs = 0, nstat = 1, nchunks = 0;
    std::vector<double> Wb, Wr;  // W_b and the sum of W sqrt(m2), of the weights in use
    double sumw2 = 0.0;
    bool has_w = false, user_w = false, ran = false;
    double2 *spec = nullptr;  // the transforms of the fields: F * comps (cross) or comps (auto) of P * H
    double2 *S = nullptr;     // one real spectrum
    double *R1 = nullptr, *R2 = nullptr;  // P^2 each: the inverses; R1 also the padded field, R2 the f32 padded weights
    double *W64 = nullptr;                // the padded weights in f64
    double *e2 = nullptr, *partial = nullptr, *sums = nullptr, *norm = nullptr;
    double *win = nullptr, *Wwin = nullptr;  // (2L+1)^2 each: slicer_xi_correlation's window, and that of W(r)
    unsigned long long *bad = nullptr;
    SLICER_FFT_INTERNAL ~slicer_xi_s() { slicer_fft_destroy(fft); }
};

int slicer_xi_bins(int32_t npix, int32_t n_edges, const double *edges, int64_t *counts, int64_t *lags, int32_t *padded)
{
    if (npix < 2 || npix >= kMaxP)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_xi_bins: npix = %d outside 2..%d", npix, kMaxP - 1);
    XiGeom g;
    const char *why = xi_geom(npix, n_edges, edges, g);
    if (*why)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_xi_bins: %s", why);
    if (g.B > SLICER_XI_MAX_BINS)
        return fail(nullptr, SLICER_ERR_UNSUPPORTED, "slicer_xi_bins: %d bins, at most %d", g.B, SLICER_XI_MAX_BINS);
    if (!g.P)
        return fail(nullptr, SLICER_ERR_UNSUPPORTED, "slicer_xi_bins: no transform size up to %d holds npix + L = %d + %d",
                    kMaxP, g.n, g.L);
    if (padded)
        *padded = g.P;
    if (counts || lags) {
        xi_enumerate(g);
        if (counts)
            std::copy(g.counts.begin(), g.counts.end(), counts);
        if (lags)
            std::copy(g.lags.begin(), g.lags.end(), lags);
    }
    return SLICER_OK;
}

namespace {

int pair_of(int s, int t, int S) { return s * S - s * (s - 1) / 2 + (t - s); }

// partial -> sums[slot .. slot + count)
int sum_launch(slicer_xi_handle xh, hipStream_t st, int count, int slot)
{
    hipLaunchKernelGGL(k_xi_sum, dim3((unsigned)((count + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads), 0, st,
                       xh->partial, xh->nchunks, count, xh->sums + slot);
    HIPCHK(xh->h, hipGetLastError());
    return SLICER_OK;
}

int bin_launch(slicer_xi_handle xh, hipStream_t st, int mode, int slot)
{
    XiBinArgs a{};
    a.r1 = xh->R1;
    a.r2 = xh->R2;
    a.e2 = xh->e2;
    a.partial = xh->partial;
    a.P = xh->g.P;
    a.L = xh->g.L;
    a.B = xh->g.B;
    a.nchunks = xh->nchunks;
    a.mode = mode;
    hipLaunchKernelGGL(k_xi_bin, dim3((unsigned)xh->nchunks, (unsigned)xh->g.B), dim3(kXiCols), 0, st, a);
    HIPCHK(xh->h, hipGetLastError());
    return sum_launch(xh, st, (mode == BIN_WEIGHT ? 2 : 1) * xh->g.B, slot);
}

// out = irfft2 of the real spectrum `mode` of the field transforms a and b (comps each)
int correlate(slicer_xi_handle xh, hipStream_t st, const double2 *a, const double2 *b, int mode, double *out)
{
    const size_t stride = (size_t)xh->g.P * (xh->g.P / 2 + 1);
    const bool two = mode != SPEC_0;
    hipLaunchKernelGGL(k_xi_spectra, dim3(groups_for(stride)), dim3(kThreads), 0, st, a, two ? a + stride : nullptr, b,
                       two ? b + stride : nullptr, xh->S, stride, mode);
    HIPCHK(xh->h, hipGetLastError());
    return slicer_fft_inverse_band(xh->fft, st, xh->S, 0.0, INFINITY, 1, out, 1);
}

// The statistics of the pair of field transforms (a, b) into the sums of pair p
int pair_launch(slicer_xi_handle xh, hipStream_t st, const double2 *a, const double2 *b, int p)
{
    const int B = xh->g.B;
    if (int rc = correlate(xh, st, a, b, xh->spin ? SPEC_PLUS : SPEC_0, xh->R1))
        return rc;
    if (int rc = bin_launch(xh, st, BIN_PLAIN, (2 + p) * B))
        return rc;
    if (!xh->spin)
        return SLICER_OK;
    if (int rc = correlate(xh, st, a, b, SPEC_MINUS, xh->R1))
        return rc;
    if (int rc = correlate(xh, st, a, b, SPEC_CROSS, xh->R2))
        return rc;
    return bin_launch(xh, st, BIN_SPIN4, (2 + xh->npairs + p) * B);
}

}  // namespace

int slicer_xi_create(slicer_handle h, int32_t npix, int32_t spin, int32_t n_fields, int32_t cross, int32_t n_edges,
                     const double *edges, slicer_xi_handle *out)
{
    const char *who = "slicer_xi_create";
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_create: null argument");
    *out = nullptr;
    if (npix < 2 || npix >= kMaxP)
        return fail(h, npix < 2 ? SLICER_ERR_ARG : SLICER_ERR_UNSUPPORTED, "slicer_xi_create: npix = %d outside 2..%d", npix,
                    kMaxP - 1);
    if (spin != 0 && spin != 2)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_create: spin = %d, expected 0 or 2", spin);
    if (n_fields < 1 || n_fields > kMaxFields)
        return fail(h, n_fields < 1 ? SLICER_ERR_ARG : SLICER_ERR_UNSUPPORTED,
                    "slicer_xi_create: n_fields = %d outside 1..%d", n_fields, kMaxFields);
    if (cross != 0 && cross != 1)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_create: cross = %d, expected 0 or 1", cross);
    XiGeom g;
    const char *why = xi_geom(npix, n_edges, edges, g);
    if (*why)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_create: %s", why);
    if (g.B > SLICER_XI_MAX_BINS)
        return fail(h, SLICER_ERR_UNSUPPORTED, "slicer_xi_create: %d bins, at most %d", g.B, SLICER_XI_MAX_BINS);
    if (!g.P)
        return fail(h, SLICER_ERR_UNSUPPORTED,
                    "slicer_xi_create: no transform size up to %d holds npix + L = %d + %d", kMaxP, g.n, g.L);
    xi_enumerate(g);
    hipStream_t st = nullptr;
    slicer_xi_handle xh = nullptr;
    if (int rc = sub_new(h, who, &st, &xh))
        return rc;
    const int B = g.B, P = g.P, L = g.L;
    xh->g = g;
    xh->spin = spin;
    xh->comps = spin ? 2 : 1;
    xh->F = n_fields;
    xh->cross = cross;
    xh->npairs = cross ? n_fields * (n_fields + 1) / 2 : n_fields;
    xh->nstat = spin ? 2 : 1;
    xh->nchunks = (2 * L + 1 + kXiCols - 1) / kXiCols;
    const size_t stride = (size_t)P * (P / 2 + 1), px = (size_t)P * P, win = (size_t)(2 * L + 1) * (2 * L + 1);
    int rc = slicer_fft_create(h, P, h->opt.shear_split, st, xh->device, who, &xh->fft);
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->spec, (size_t)(cross ? n_fields : 1) * xh->comps * stride * sizeof(double2));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->S, stride * sizeof(double2));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->R1, px * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->R2, px * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->W64, px * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->win, win * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->Wwin, win * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->e2, (B + 1) * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->partial, (size_t)2 * B * xh->nchunks * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->sums, (size_t)(2 + xh->nstat * xh->npairs) * B * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->norm, kNormGroups * sizeof(double));
    rc = xh->mem.alloc(rc, h, who, (void **)&xh->bad, kNormGroups * sizeof(unsigned long long));
    if (rc == SLICER_OK) {
        hipError_t e = hipMemcpyAsync(xh->e2, xh->g.e2.data(), (B + 1) * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "slicer_xi_create: upload: %s", hipGetErrorString(e));
    }
    if (rc == SLICER_OK)
        rc = slicer_xi_set_weights(xh, nullptr);
    return sub_done(rc, xh, out);
}

int slicer_xi_set_weights(slicer_xi_handle xh, const float *d_w)
{
    if (!xh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_xi_set_weights: null handle");
    slicer_handle h = xh->h;
    hipStream_t st;
    if (int rc = sub_stream(h, xh->device, &st))
        return rc;
    xh->has_w = xh->ran = false;
    const int n = xh->g.n, P = xh->g.P, B = xh->g.B, L = xh->g.L;
    const size_t px = (size_t)P * P;
    if (d_w) {
        hipLaunchKernelGGL(k_xi_norm, dim3(kNormGroups), dim3(kThreads), 0, st, d_w, (size_t)n * n, xh->norm, xh->bad);
        HIPCHK(h, hipGetLastError());
        std::vector<double> part(kNormGroups);
        std::vector<unsigned long long> bad(kNormGroups);
        HIPCHK(h, hipMemcpyAsync(part.data(), xh->norm, kNormGroups * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(bad.data(), xh->bad, kNormGroups * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        double s2 = 0.0;
        unsigned long long nbad = 0;
        for (int g = 0; g < kNormGroups; g++) {
            s2 += part[g];
            nbad += bad[g];
        }
        if (nbad)
            return fail(h, SLICER_ERR_ARG, "slicer_xi_set_weights: the weights have %llu values that are negative or not finite",
                        nbad);
        xh->sumw2 = s2;
    } else {
        xh->sumw2 = (double)n * (double)n;
    }
    hipLaunchKernelGGL(k_xi_pad<double>, dim3(groups_for(px)), dim3(kThreads), 0, st, d_w, xh->W64, n, P);
    HIPCHK(h, hipGetLastError());
    xh->Wb.resize(B);
    xh->Wr.resize(B);
    if (d_w) {
        float *w32 = (float *)xh->R2;
        hipLaunchKernelGGL(k_xi_pad<float>, dim3(groups_for(px)), dim3(kThreads), 0, st, d_w, w32, n, P);
        HIPCHK(h, hipGetLastError());
        if (int rc = slicer_fft_forward(xh->fft, st, w32, xh->S))
            return rc;
        if (int rc = correlate(xh, st, xh->S, xh->S, SPEC_0, xh->R1))
            return rc;
        if (int rc = bin_launch(xh, st, BIN_WEIGHT, 0))
            return rc;
        hipLaunchKernelGGL(k_xi_window, dim3(groups_for((size_t)(2 * L + 1) * (2 * L + 1))), dim3(kThreads), 0, st, xh->R1,
                           xh->Wwin, P, L);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(xh->Wb.data(), xh->sums, B * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemcpyAsync(xh->Wr.data(), xh->sums + B, B * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    } else {
        for (int b = 0; b < B; b++) {
            xh->Wb[b] = (double)xh->g.counts[b];
            xh->Wr[b] = xh->g.nr[b];
        }
    }
    xh->user_w = d_w != nullptr;
    xh->has_w = true;
    return SLICER_OK;
}

int slicer_xi_run(slicer_xi_handle xh, const float *const *d_maps)
{
    if (!xh || !d_maps)
        return fail(xh ? xh->h : nullptr, SLICER_ERR_ARG, "slicer_xi_run: null argument");
    slicer_handle h = xh->h;
    const int nmaps = xh->F * xh->comps;
    for (int s = 0; s < nmaps; s++)
        if (!d_maps[s])
            return fail(h, SLICER_ERR_ARG, "slicer_xi_run: map %d is null", s);
    if (!xh->has_w)
        return fail(h, SLICER_ERR_STATE, "slicer_xi_run after a refused slicer_xi_set_weights");
    hipStream_t st;
    if (int rc = sub_stream(h, xh->device, &st))
        return rc;
    xh->ran = false;
    const int n = xh->g.n, P = xh->g.P, comps = xh->comps;
    const size_t px = (size_t)P * P, stride = (size_t)P * (P / 2 + 1);
    auto forward = [&](int f) {
        for (int c = 0; c < comps; c++) {
            hipLaunchKernelGGL(k_xi_pad<double>, dim3(groups_for(px)), dim3(kThreads), 0, st, d_maps[f * comps + c], xh->R1,
                               n, P);
            HIPCHK(h, hipGetLastError());
            double2 *khat = xh->spec + ((size_t)(xh->cross ? f : 0) * comps + c) * stride;
            if (int rc = slicer_fft_forward_product(xh->fft, st, xh->R1, xh->W64, khat))
                return rc;
        }
        return (int)SLICER_OK;
    };
    if (xh->cross) {
        for (int f = 0; f < xh->F; f++)
            if (int rc = forward(f))
                return rc;
        for (int s = 0; s < xh->F; s++)
            for (int t = s; t < xh->F; t++)
                if (int rc = pair_launch(xh, st, xh->spec + (size_t)s * comps * stride, xh->spec + (size_t)t * comps * stride,
                                         pair_of(s, t, xh->F)))
                    return rc;
    } else {
        for (int f = 0; f < xh->F; f++) {
            if (int rc = forward(f))
                return rc;
            if (int rc = pair_launch(xh, st, xh->spec, xh->spec, f))
                return rc;
        }
    }
    xh->ran = true;
    return SLICER_OK;
}

int slicer_xi_read(slicer_xi_handle xh, double *xi, double *xim, double *r_mean, double *weights, int64_t *counts)
{
    if (!xh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_xi_read: null handle");
    slicer_handle h = xh->h;
    if (!xh->ran)
        return fail(h, SLICER_ERR_STATE, "slicer_xi_read before any slicer_xi_run");
    if (xim && !xh->spin)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_read: xim of a spin-0 handle");
    const int B = xh->g.B, np = xh->npairs;
    std::vector<double> sums((size_t)xh->nstat * np * B);
    if (int rc = sub_read(*xh, sums.data(), xh->sums + 2 * B, sums.size() * sizeof(double)))
        return rc;
    const double floor_w = std::ldexp(xh->sumw2, -30);
    for (int b = 0; b < B; b++) {
        const bool empty = xh->g.lags[b] == 0 || !(xh->Wb[b] > floor_w);
        for (int p = 0; p < np; p++) {
            if (xi)
                xi[(size_t)p * B + b] = empty ? NAN : sums[(size_t)p * B + b] / xh->Wb[b];
            if (xim)
                xim[(size_t)p * B + b] = empty ? NAN : sums[(size_t)(np + p) * B + b] / xh->Wb[b];
        }
        if (r_mean)
            r_mean[b] = empty ? NAN : xh->Wr[b] / xh->Wb[b];
        if (weights)
            weights[b] = xh->Wb[b];
        if (counts)
            counts[b] = xh->g.counts[b];
    }
    return SLICER_OK;
}

int slicer_xi_correlation(slicer_xi_handle xh, int32_t pair, int32_t which, double *host)
{
    if (!xh || !host)
        return fail(xh ? xh->h : nullptr, SLICER_ERR_ARG, "slicer_xi_correlation: null argument");
    slicer_handle h = xh->h;
    const int L = xh->g.L, n = xh->g.n, P = xh->g.P, W = 2 * L + 1;
    const size_t win = (size_t)W * W;
    if (which == SLICER_XI_WEIGHTS) {
        if (!xh->has_w)
            return fail(h, SLICER_ERR_STATE, "slicer_xi_correlation after a refused slicer_xi_set_weights");
        if (xh->user_w)
            return sub_read(*xh, host, xh->Wwin, win * sizeof(double));
        for (int dx = -L; dx <= L; dx++)
            for (int dy = -L; dy <= L; dy++)
                host[(size_t)(dx + L) * W + (dy + L)] = (double)(n - std::abs(dx)) * (double)(n - std::abs(dy));
        return SLICER_OK;
    }
    if (which < 0 || which > (xh->spin ? SLICER_XI_CROSS : SLICER_XI_PLUS))
        return fail(h, SLICER_ERR_ARG, "slicer_xi_correlation: which = %d outside 0..%d of spin %d, and not the weights", which,
                    xh->spin ? SLICER_XI_CROSS : SLICER_XI_PLUS, xh->spin);
    if (pair < 0 || pair >= xh->npairs)
        return fail(h, SLICER_ERR_ARG, "slicer_xi_correlation: pair = %d outside 0..%d", pair, xh->npairs - 1);
    if (!xh->ran)
        return fail(h, SLICER_ERR_STATE, "slicer_xi_correlation before any slicer_xi_run");
    if (!xh->cross && pair != xh->F - 1)
        return fail(h, SLICER_ERR_STATE, "slicer_xi_correlation: auto mode keeps only the last field's transforms");
    hipStream_t st;
    if (int rc = sub_stream(h, xh->device, &st))
        return rc;
    int s = 0, t = 0;
    if (xh->cross) {
        int rem = pair;
        while (rem >= xh->F - s) {
            rem -= xh->F - s;
            s++;
        }
        t = s + rem;
    }
    const size_t fs = (size_t)xh->comps * P * (P / 2 + 1);
    const int mode = !xh->spin ? SPEC_0 : which == SLICER_XI_PLUS ? SPEC_PLUS : which == SLICER_XI_MINUS ? SPEC_MINUS : SPEC_CROSS;
    if (int rc = correlate(xh, st, xh->spec + s * fs, xh->spec + t * fs, mode, xh->R1))
        return rc;
    hipLaunchKernelGGL(k_xi_window, dim3(groups_for(win)), dim3(kThreads), 0, st, xh->R1, xh->win, P, L);
    HIPCHK(h, hipGetLastError());
    return sub_read(*xh, host, xh->win, win * sizeof(double));
}

int slicer_xi_destroy(slicer_xi_handle xh) { return sub_destroy(xh); }
