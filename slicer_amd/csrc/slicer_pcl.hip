// slicer_pcl.hip -- on-device masked pseudo-C_l of kappa maps: coupled bandpowers, the mode-coupling matrix of the mask
// and the decoupled bandpowers (the definitions are in include/slicer_amd.h).
//
// The handle is built on a power handle (slicer_power.hip, row N7), whose plan, bins, slices and binning kernels it
// uses through slicer_power_internal.hpp; the transforms are those of slicer_fft.hip:
//   run       slicer_power_run_masked: the forward transforms load w * kappa (slicer_fft_forward_masked), the rest is
//             slicer_power_run, so the spectra and the coupled bandpowers are bitwise those of the multiplied maps
//   set_mask  k_pcl_mask builds w from the taper table and the user mask; k_pcl_moments sums w, w^2 and counts the
//             values that are not finite; A = irfft2(|rfft2 w|^2) (slicer_fft_forward, slicer_fft_inverse_abs2); then per
//             non-empty bin b': G = irfft2(1[F_b']) (slicer_fft_inverse_band with the DC mode kept), Q = rfft2(A G)
//             (slicer_fft_forward_product) and column b' of M from the binning of Re Q (slicer_power_bin_real)
//   read      the LU of the active part of M (slicer_pcl_internal.hpp), factorised by set_mask on the host, applied to the
//             coupled bandpowers
// No atomics: the moments are per-workgroup partials in a fixed tree, summed in workgroup order on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "slicer_power_internal.hpp"
#include "slicer_host.hpp"
#include "slicer_pcl_internal.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMomentGroups = kPclMomentGroups;

// w = (float)(f[i0] * f[i1]) (1 without a table), times the user mask in f32 where there is one
__global__ __launch_bounds__(kThreads) void k_pcl_mask(const double *f, const float *user, float *w, int n)
{
    const size_t total = (size_t)n * n;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int i0 = (int)(i / n), i1 = (int)(i - (size_t)i0 * n);
        float v = f ? (float)(f[i0] * f[i1]) : 1.0f;
        if (user)
            v = f ? v * user[i] : user[i];
        w[i] = v;
    }
}

// partial[g] = {sum of w, sum of w^2} over the finite pixels i = g * 256 + t + k * 256 * groups, bad[g] = the number of
// the others; every thread sums its pixels in index order, the workgroup in a fixed tree
__global__ __launch_bounds__(kThreads) void k_pcl_moments(const float *w, size_t total, double2 *partial,
                                                          unsigned long long *bad)
{
    __shared__ double s1[kThreads], s2[kThreads];
    __shared__ unsigned long long sb[kThreads];
    double a = 0.0, b = 0.0;
    unsigned long long nb = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const double v = (double)w[i];
        if (isfinite(v)) {
            a += v;
            b += v * v;
        } else {
            nb++;
        }
    }
    const int t = threadIdx.x;
    s1[t] = a;
    s2[t] = b;
    sb[t] = nb;
    __syncthreads();
    for (int d = kThreads / 2; d >= 1; d /= 2) {
        if (t < d) {
            s1[t] += s1[t + d];
            s2[t] += s2[t + d];
            sb[t] += sb[t + d];
        }
        __syncthreads();
    }
    if (t == 0) {
        partial[blockIdx.x] = make_double2(s1[0], s2[0]);
        bad[blockIdx.x] = sb[0];
    }
}

}  // namespace

struct slicer_pcl_s : SubHandle {
    slicer_power_handle pw = nullptr;  // plan, bins, slices, spectra and coupled bandpowers
    int n = 0, S = 0, cross = 0, B = 0, npairs = 0;
    std::vector<double> e2;           // edge squares, B + 1
    std::vector<int64_t> counts;      // N_b
    std::vector<int> active;          // the bins with N_b > 0
    std::vector<double> M;            // [B][B]
    std::vector<double> lu;           // the LU of M's active part, [na][na], unit lower triangle below the diagonal
    std::vector<int> piv;             // row exchanged with row k at step k
    double mean_w = 0.0, mean_w2 = 0.0;
    float *w = nullptr;
    double *A = nullptr, *G = nullptr, *f = nullptr, *Mt = nullptr;  // Mt: [b'][b], as the columns are binned
    double2 *Q = nullptr, *partial = nullptr;
    unsigned long long *bad = nullptr;
    bool has_mask = false, ran = false;
    SLICER_FFT_INTERNAL ~slicer_pcl_s()
    {
        if (pw)
            slicer_power_destroy(pw);
    }
};

int slicer_pcl_taper(int32_t npix, double width_pix, double *f)
{
    if (npix < 2 || !f)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl_taper: npix below 2, or null output");
    if (!std::isfinite(width_pix) || width_pix <= 0.0)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl_taper: the width must be positive and finite");
    for (int i = 0; i < npix; i++) {
        const double x = (double)std::min(i, npix - 1 - i) + 0.5, t = x / width_pix;
        f[i] = t >= 1.0 ? 1.0 : t - std::sin(2.0 * M_PI * t) / (2.0 * M_PI);
    }
    return SLICER_OK;
}

int slicer_pcl_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_maps, int32_t cross, int32_t n_edges,
                      const double *edges, slicer_pcl_handle *out)
{
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl_create: null argument");
    *out = nullptr;
    if (!edges)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl_create: the edges are required");
    if (n_edges - 1 > SLICER_PCL_MAX_BINS)
        return fail(h, SLICER_ERR_UNSUPPORTED, "slicer_pcl_create: %d bins, at most %d", n_edges - 1, SLICER_PCL_MAX_BINS);
    slicer_power_handle pw = nullptr;
    if (int rc = slicer_power_create(h, npix, angle_deg, n_maps, cross, n_edges, edges, &pw)) {
        // the refusals of slicer_power_create under this call's name
        std::string why = slicer_last_error(h);
        const std::string pre = "slicer_power_create";
        if (why.compare(0, pre.size(), pre) == 0)
            why = "slicer_pcl_create" + why.substr(pre.size());
        return fail(h, rc, "%s", why.c_str());
    }
    const char *who = "slicer_pcl_create";
    hipStream_t st = nullptr;
    slicer_pcl_handle ph = nullptr;
    if (int rc = sub_new(h, who, &st, &ph)) {
        slicer_power_destroy(pw);
        return rc;
    }
    const int n = npix, B = n_edges - 1;
    ph->pw = pw;
    ph->n = n;
    ph->S = n_maps;
    ph->cross = cross;
    ph->B = B;
    ph->npairs = cross ? n_maps * (n_maps + 1) / 2 : n_maps;
    ph->e2.resize(B + 1);
    for (int b = 0; b <= B; b++)
        ph->e2[b] = edges[b] * edges[b];
    ph->counts.resize(B);
    std::vector<double> mean(B);
    int rc = slicer_power_bins(n, n_edges, edges, ph->counts.data(), mean.data());
    for (int b = 0; b < B; b++)
        if (ph->counts[b] > 0)
            ph->active.push_back(b);
    const size_t px = (size_t)n * n;
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->w, px * sizeof(float));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->A, px * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->G, px * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Q, (size_t)n * (n / 2 + 1) * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->f, (size_t)n * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Mt, (size_t)B * B * sizeof(double), &st);
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->partial, kMomentGroups * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->bad, kMomentGroups * sizeof(unsigned long long));
    return sub_done(rc, ph, out);
}

int pcl_build_mask(slicer_handle h, const char *who, hipStream_t st, int n, const float *d_mask, double taper_width_pix,
                   float *d_w, double *d_f, double2 *d_partial, unsigned long long *d_bad, double *mean_w, double *mean_w2)
{
    const size_t px = (size_t)n * n;
    const bool taper = taper_width_pix > 0.0;
    std::vector<double> f;
    if (taper) {
        f.resize(n);
        if (int rc = slicer_pcl_taper(n, taper_width_pix, f.data()))
            return fail(h, rc, "%s", slicer_last_error(nullptr));
        HIPCHK(h, hipMemcpyAsync(d_f, f.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const unsigned groups = (unsigned)std::min<size_t>(4096, (px + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_pcl_mask, dim3(groups), dim3(kThreads), 0, st, taper ? d_f : nullptr, d_mask, d_w, n);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_pcl_moments, dim3(kMomentGroups), dim3(kThreads), 0, st, d_w, px, d_partial, d_bad);
    HIPCHK(h, hipGetLastError());
    std::vector<double2> part(kMomentGroups);
    std::vector<unsigned long long> bad(kMomentGroups);
    HIPCHK(h, hipMemcpyAsync(part.data(), d_partial, kMomentGroups * sizeof(double2), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(bad.data(), d_bad, kMomentGroups * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));  // also: f is a host temporary
    double s1 = 0.0, s2 = 0.0;
    unsigned long long nbad = 0;
    for (int g = 0; g < kMomentGroups; g++) {
        s1 += part[g].x;
        s2 += part[g].y;
        nbad += bad[g];
    }
    if (nbad)
        return fail(h, SLICER_ERR_ARG, "%s: the mask has %llu values that are not finite", who, nbad);
    *mean_w = s1 / (double)px;
    *mean_w2 = s2 / (double)px;
    return SLICER_OK;
}

int slicer_pcl_set_mask(slicer_pcl_handle ph, const float *d_mask, double taper_width_pix)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl_set_mask: null handle");
    slicer_handle h = ph->h;
    if (!std::isfinite(taper_width_pix) || taper_width_pix < 0.0)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl_set_mask: the taper width must be finite and not negative");
    const bool taper = taper_width_pix > 0.0;
    if (!d_mask && !taper)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl_set_mask: neither a mask nor a taper");
    hipStream_t st;
    if (int rc = sub_stream(h, ph->device, &st))
        return rc;
    ph->has_mask = ph->ran = false;
    const int n = ph->n, B = ph->B;
    if (int rc = pcl_build_mask(h, "slicer_pcl_set_mask", st, n, d_mask, taper_width_pix, ph->w, ph->f, ph->partial,
                                ph->bad, &ph->mean_w, &ph->mean_w2))
        return rc;

    // A, then M column by column
    slicer_fft_s *plan = slicer_power_plan(ph->pw);
    if (int rc = slicer_fft_forward(plan, st, ph->w, ph->Q))
        return rc;
    if (int rc = slicer_fft_inverse_abs2(plan, st, ph->Q, ph->A))
        return rc;
    const double norm = 1.0 / ((double)n * (double)n);
    for (int b : ph->active) {
        if (int rc = slicer_fft_inverse_band(plan, st, nullptr, ph->e2[b], ph->e2[b + 1], b == B - 1, ph->G, 1))
            return rc;
        if (int rc = slicer_fft_forward_product(plan, st, ph->A, ph->G, ph->Q))
            return rc;
        if (int rc = slicer_power_bin_real(ph->pw, st, ph->Q, norm, b, ph->Mt))
            return rc;
    }
    std::vector<double> Mt((size_t)B * B);
    HIPCHK(h, hipMemcpyAsync(Mt.data(), ph->Mt, Mt.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    ph->M.assign((size_t)B * B, 0.0);
    for (int b : ph->active)
        for (int c : ph->active)
            ph->M[(size_t)b * B + c] = Mt[(size_t)c * B + b];
    const int na = (int)ph->active.size();
    ph->lu.resize((size_t)na * na);
    for (int i = 0; i < na; i++)
        for (int j = 0; j < na; j++)
            ph->lu[(size_t)i * na + j] = ph->M[(size_t)ph->active[i] * B + ph->active[j]];
    if (!lu_factor(ph->lu, na, ph->piv))
        return fail(h, SLICER_ERR_ARG, "slicer_pcl_set_mask: coupling matrix singular");
    ph->has_mask = true;
    return SLICER_OK;
}

int slicer_pcl_read_mask(slicer_pcl_handle ph, float *host)
{
    if (!ph || !host)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl_read_mask: null argument");
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_read_mask before any slicer_pcl_set_mask");
    return sub_read(*ph, host, ph->w, (size_t)ph->n * ph->n * sizeof(float));
}

int slicer_pcl_coupling(slicer_pcl_handle ph, double *M, double *mean_w, double *mean_w2)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl_coupling: null handle");
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_coupling before any slicer_pcl_set_mask");
    if (M)
        std::copy(ph->M.begin(), ph->M.end(), M);
    if (mean_w)
        *mean_w = ph->mean_w;
    if (mean_w2)
        *mean_w2 = ph->mean_w2;
    return SLICER_OK;
}

int slicer_pcl_run(slicer_pcl_handle ph, const float *const *d_maps)
{
    if (!ph || !d_maps)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl_run: null argument");
    for (int s = 0; s < ph->S; s++)
        if (!d_maps[s])
            return fail(ph->h, SLICER_ERR_ARG, "slicer_pcl_run: map %d is null", s);
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_run before any slicer_pcl_set_mask");
    ph->ran = false;
    if (int rc = slicer_power_run_masked(ph->pw, d_maps, ph->w))
        return rc;
    ph->ran = true;
    return SLICER_OK;
}

int slicer_pcl_spectrum(slicer_pcl_handle ph, int32_t map, double *host)
{
    if (!ph || !host)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl_spectrum: null argument");
    if (map < 0 || map >= ph->S)
        return fail(ph->h, SLICER_ERR_ARG, "slicer_pcl_spectrum: map = %d outside 0..%d", map, ph->S - 1);
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_spectrum before any slicer_pcl_run");
    if (!ph->cross && map != ph->S - 1)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_spectrum: auto mode keeps only the last map's spectrum");
    return slicer_power_spectrum(ph->pw, map, host);
}

int slicer_pcl_read(slicer_pcl_handle ph, double *cl, double *coupled, double *ell_mean, int64_t *counts)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl_read: null handle");
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl_read before any slicer_pcl_run");
    const int B = ph->B, na = (int)ph->active.size();
    std::vector<double> own;
    double *ct = coupled;
    if (cl && !ct) {
        own.resize((size_t)ph->npairs * B);
        ct = own.data();
    }
    if (int rc = slicer_power_read(ph->pw, ct, ell_mean, counts))
        return rc;
    if (cl) {
        std::vector<double> x(na);
        for (int p = 0; p < ph->npairs; p++) {
            for (int i = 0; i < na; i++)
                x[i] = ct[(size_t)p * B + ph->active[i]];
            lu_solve(ph->lu, na, ph->piv, x.data());
            for (int b = 0; b < B; b++)
                cl[(size_t)p * B + b] = NAN;
            for (int i = 0; i < na; i++)
                cl[(size_t)p * B + ph->active[i]] = x[i];
        }
    }
    return SLICER_OK;
}

int slicer_pcl_destroy(slicer_pcl_handle ph) { return sub_destroy(ph); }
