// slicer_scattering.hip -- on-device wavelet scattering coefficients of a kappa map, orders 0, 1 and 2 (DESIGN.md S8
// row N20; the filters, the transform and the outputs are defined in include/slicer_amd.h).
//
// Every W_{jl} f = |ifft2(fhat psi^_{jl})| is the modulus of a complex field, and slicer_fft.hip has real transforms only.
// psi^ is real, so with E and O its even and odd parts under negation of the mode index, fhat E and -i fhat O are both
// Hermitian: x = irfft2(fhat E) and y = irfft2(-i fhat O) are the real and imaginary parts of the complex field.
//   run   khat = rfft2(kappa) (slicer_fft_forward), s0 (k_scat_sums of the map itself); per (j1, l1): k_scat_filter
//         (khat E, -i khat O), two slicer_fft_inverse_band with every mode kept (x, y), k_scat_sums and k_scat_finish (s1,
//         p1), slicer_fft_forward_hypot (u1hat; u1 itself is never stored); then per (j2 > j1, l2) the same on u1hat (s2).
//         x and y are reused by every transform.  Nothing is subsampled: every field keeps n^2 pixels.
//   read  the means from the device, NaN where j2 <= j1
// k_scat_filter: one thread per half-plane mode [a][b <= n/2] (grid-stride).  It evaluates psi^ at the mode and at the
// negated index on the fly, 18 exp each (scat_psi of slicer_scattering_filter.hpp, the expression of the host's
// slicer_scattering_filter): no n^2 filter tables.  At a self-conjugate mode both evaluations are the same, O = 0.
// k_scat_sums: the sums of u and u^2, u = sqrt(x x + y y), in the fixed order of k_bispectrum: a wave owns one chunk of
// pixels, a lane sums blocks of kInner values (64 pixels apart) in registers and adds every block to a second
// accumulator, one xor butterfly ends the chunk.  k_scat_finish: lane l adds a contiguous run of the chunks in index
// order, then the same butterfly, and stores sum / n^2.  No atomics; no load wider than its element, so a map pointer
// off the 16-byte grid takes the same path: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_fft.hpp"
#include "slicer_host.hpp"
#include "slicer_scattering_filter.hpp"

namespace {

constexpr int kMaxJ = SLICER_SCATTERING_MAX_J, kMaxL = SLICER_SCATTERING_MAX_L;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kInner = 64;       // values of a lane's inner block
constexpr int kMinChunk = 8192;  // pixels per chunk, at least; at most kMaxChunks chunks
constexpr int kMaxChunks = 4096;
constexpr int kFilterPerCu = 8;  // workgroups of k_scat_filter per CU, at most

// p1 = spec * E, p2 = -i * spec * O over the [n][H] half plane
__global__ __launch_bounds__(kThreads) void k_scat_filter(const double2 *spec, double2 *p1, double2 *p2, int n, int H,
                                                          ScatFilter f)
{
    const size_t total = (size_t)n * H;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int a = (int)(i / H), b = (int)(i - (size_t)a * H);
        const double psi = scat_psi(f, n, a, b), neg = scat_psi(f, n, a ? n - a : 0, b ? n - b : 0);
        const double E = (psi + neg) / 2.0, O = (psi - neg) / 2.0;
        const double2 s = spec[i];
        p1[i] = make_double2(s.x * E, s.y * E);
        p2[i] = make_double2(s.y * O, -(s.x * O));
    }
}

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off /= 2)
        v += __shfl_xor(v, off, 64);
    return v;
}

// partial[c] = the sum of v, partial[nchunks + c] = the sum of v * v over chunk c.  MAP: v = (double)map[i];
// otherwise v = sqrt(x[i] x[i] + y[i] y[i]).  chunk is a multiple of 64.
template <bool MAP>
__global__ __launch_bounds__(kThreads) void k_scat_sums(const float *map, const double *x, const double *y, size_t n2,
                                                        int chunk, int nchunks, double *partial)
{
    const int lane = threadIdx.x % 64, c = (int)blockIdx.x * kWaves + threadIdx.x / 64;
    if (c >= nchunks)
        return;
    const size_t i0 = (size_t)c * chunk + lane;
    const int steps = chunk / 64;
    double outer0 = 0.0, outer1 = 0.0;
    for (int b0 = 0; b0 < steps; b0 += kInner) {
        const int b1 = min(b0 + kInner, steps);
        double acc0 = 0.0, acc1 = 0.0;
        for (int b = b0; b < b1; b++) {
            const size_t i = i0 + (size_t)b * 64;
            double v = 0.0;
            if (i < n2) {
                if (MAP) {
                    v = (double)map[i];
                } else {
                    const double xv = x[i], yv = y[i];
                    v = sqrt(xv * xv + yv * yv);
                }
            }
            acc0 += v;
            acc1 += v * v;
        }
        outer0 = b0 == 0 ? acc0 : outer0 + acc0;
        outer1 = b0 == 0 ? acc1 : outer1 + acc1;
    }
    outer0 = wave_sum(outer0);
    outer1 = wave_sum(outer1);
    if (lane == 0) {
        partial[c] = outer0;
        partial[nchunks + c] = outer1;
    }
}

// out[0] = (the chunks' first sums) / n2 and, unless out2 is null, out2[0] = (their second sums) / n2: wave w of the
// one workgroup takes value w, lane l adds chunks l per ... (l + 1) per - 1 in order
__global__ __launch_bounds__(128) void k_scat_finish(const double *partial, int nchunks, double n2, double *out,
                                                     double *out2)
{
    const int lane = threadIdx.x % 64, w = threadIdx.x / 64;
    const int per = (nchunks + 63) / 64, c0 = min(lane * per, nchunks), c1 = min(c0 + per, nchunks);
    double v = 0.0;
    for (int c = c0; c < c1; c++)
        v += partial[(size_t)w * nchunks + c];
    v = wave_sum(v);
    if (lane == 0) {
        if (w == 0)
            out[0] = v / n2;
        else if (out2)
            out2[0] = v / n2;
    }
}

// x[i] = sqrt(x[i]^2 + y[i]^2): the field slicer_scattering_modulus returns
__global__ __launch_bounds__(kThreads) void k_scat_modulus(double *x, const double *y, size_t n2)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n2; i += (size_t)gridDim.x * kThreads) {
        const double xv = x[i], yv = y[i];
        x[i] = sqrt(xv * xv + yv * yv);
    }
}

ScatFilter make_filter(int L, int j, int l)
{
    ScatFilter f{};
    const double sigma = 0.8 * std::ldexp(1.0, j), s = 4.0 / (double)L, theta = M_PI * (double)l / (double)L;
    f.h = sigma * sigma / 2.0;
    f.xi = (3.0 * M_PI / 4.0) * std::ldexp(1.0, -j);
    f.s2 = s * s;
    f.ct = std::cos(theta);
    f.st = std::sin(theta);
    double A0, B0;
    scat_alias_sums(f, 0.0, 0.0, A0, B0);
    f.beta = A0 / B0;
    return f;
}

// The numbers of a create or a filter call, checked before any handle; 0 or the refusal.
int check_numbers(slicer_handle h, const char *who, int npix, int J, int L)
{
    if (!fft_size_supported(npix))
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: npix = %d unsupported (2..16384, prime factors 2, 3, 5, 7 only)", who,
                    npix);
    if (J > kMaxJ)
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: J = %d above %d", who, J, kMaxJ);
    if (L > kMaxL)
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: L = %d above %d", who, L, kMaxL);
    if (J < 1)
        return fail(h, SLICER_ERR_ARG, "%s: J = %d below 1", who, J);
    if (L < 1)
        return fail(h, SLICER_ERR_ARG, "%s: L = %d below 1", who, L);
    if ((1 << J) > npix)
        return fail(h, SLICER_ERR_ARG, "%s: 2^J = %d above npix = %d", who, 1 << J, npix);
    return SLICER_OK;
}

}  // namespace

struct slicer_scattering_s : SubHandle {
    slicer_fft_s *fft = nullptr;
    int n = 0, H = 0, J = 0, L = 0, chunk = 0, nchunks = 0;
    std::vector<ScatFilter> filt;                                       // [J][L]
    double2 *khat = nullptr, *uhat = nullptr, *P1 = nullptr, *P2 = nullptr;  // n * H each
    double *X = nullptr, *Y = nullptr;                                  // n^2 each
    double *partial = nullptr;                                          // [2][nchunks]
    double *res = nullptr;  // s0 [2], then (s1, p1) [J][L][2], then s2 [J][L][J][L] (j2 <= j1 never written)
    bool ran = false;
    SLICER_FFT_INTERNAL ~slicer_scattering_s() { slicer_fft_destroy(fft); }
    size_t res_count() const { return 2 + 2 * (size_t)J * L + (size_t)J * L * J * L; }
};

namespace {

unsigned groups_for(size_t total, int per_cu, int num_cus)
{
    return (unsigned)std::min<size_t>((size_t)per_cu * (size_t)std::max(num_cus, 1), (total + kThreads - 1) / kThreads);
}

// X, Y = the real and imaginary parts of ifft2(spec_full psi^_{jl})
int transform(slicer_scattering_handle sh, hipStream_t st, const double2 *spec, int j, int l)
{
    const size_t total = (size_t)sh->n * sh->H;
    hipLaunchKernelGGL(k_scat_filter, dim3(groups_for(total, kFilterPerCu, sh->h->num_cus)), dim3(kThreads), 0, st, spec,
                       sh->P1, sh->P2, sh->n, sh->H, sh->filt[(size_t)j * sh->L + l]);
    HIPCHK(sh->h, hipGetLastError());
    if (int rc = slicer_fft_inverse_band(sh->fft, st, sh->P1, 0.0, INFINITY, 1, sh->X, 1))
        return rc;
    return slicer_fft_inverse_band(sh->fft, st, sh->P2, 0.0, INFINITY, 1, sh->Y, 1);
}

// out[0] = the mean of u, out2[0] (unless null) = the mean of u^2; u = the map, or sqrt(X^2 + Y^2) for a null map
int means(slicer_scattering_handle sh, hipStream_t st, const float *map, double *out, double *out2)
{
    const size_t n2 = (size_t)sh->n * sh->n;
    const dim3 grid((unsigned)((sh->nchunks + kWaves - 1) / kWaves));
    if (map)
        hipLaunchKernelGGL(k_scat_sums<true>, grid, dim3(kThreads), 0, st, map, nullptr, nullptr, n2, sh->chunk, sh->nchunks,
                           sh->partial);
    else
        hipLaunchKernelGGL(k_scat_sums<false>, grid, dim3(kThreads), 0, st, nullptr, sh->X, sh->Y, n2, sh->chunk,
                           sh->nchunks, sh->partial);
    HIPCHK(sh->h, hipGetLastError());
    hipLaunchKernelGGL(k_scat_finish, dim3(1), dim3(128), 0, st, sh->partial, sh->nchunks, (double)n2, out, out2);
    HIPCHK(sh->h, hipGetLastError());
    return SLICER_OK;
}

}  // namespace

int slicer_scattering_filter(int32_t npix, int32_t J, int32_t L, int32_t j, int32_t l, double *out)
{
    const char *who = "slicer_scattering_filter";
    if (int rc = check_numbers(nullptr, who, npix, J, L))
        return rc;
    if (j < 0 || j >= J || l < 0 || l >= L)
        return fail(nullptr, SLICER_ERR_ARG, "%s: (j, l) = (%d, %d) outside 0..%d, 0..%d", who, j, l, J - 1, L - 1);
    if (!out)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    const ScatFilter f = make_filter(L, j, l);
    for (int a = 0; a < npix; a++)
        for (int b = 0; b < npix; b++)
            out[(size_t)a * npix + b] = scat_psi(f, npix, a, b);
    return SLICER_OK;
}

int slicer_scattering_create(slicer_handle h, int32_t npix, int32_t J, int32_t L, slicer_scattering_handle *out)
{
    const char *who = "slicer_scattering_create";
    if (out)
        *out = nullptr;
    if (int rc = check_numbers(h, who, npix, J, L))
        return rc;
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    hipStream_t st = nullptr;
    slicer_scattering_handle sh = nullptr;
    if (int rc = sub_new(h, who, &st, &sh))
        return rc;
    const int n = npix, H = n / 2 + 1;
    sh->n = n;
    sh->H = H;
    sh->J = J;
    sh->L = L;
    for (int j = 0; j < J; j++)
        for (int l = 0; l < L; l++)
            sh->filt.push_back(make_filter(L, j, l));
    const size_t n2 = (size_t)n * n, cbytes = (size_t)n * H * sizeof(double2);
    const size_t want = std::min<size_t>(kMaxChunks, (n2 + kMinChunk - 1) / kMinChunk);
    sh->chunk = (int)(((n2 + want - 1) / want + 63) / 64 * 64);
    sh->nchunks = (int)((n2 + sh->chunk - 1) / sh->chunk);
    int rc = slicer_fft_create(h, n, h->opt.shear_split, st, sh->device, who, &sh->fft);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->khat, cbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->uhat, cbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->P1, cbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->P2, cbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->X, n2 * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->Y, n2 * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->partial, 2 * (size_t)sh->nchunks * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->res, sh->res_count() * sizeof(double), &st);
    return sub_done(rc, sh, out);
}

int slicer_scattering_run(slicer_scattering_handle sh, const float *d_map)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_scattering_run: null argument");
    slicer_handle h = sh->h;
    hipStream_t st;
    if (int rc = sub_stream(h, sh->device, &st))
        return rc;
    sh->ran = false;
    const int J = sh->J, L = sh->L, JL = J * L;
    double *first = sh->res + 2, *second = sh->res + 2 + 2 * (size_t)JL;
    {
        ProfScope ps(h, KN_SCATTERING_FIRST);
        if (int rc = slicer_fft_forward(sh->fft, st, d_map, sh->khat))
            return rc;
        if (int rc = means(sh, st, d_map, sh->res, sh->res + 1))
            return rc;
    }
    for (int j1 = 0; j1 < J; j1++)
        for (int l1 = 0; l1 < L; l1++) {
            const size_t a = (size_t)j1 * L + l1;
            {
                ProfScope ps(h, KN_SCATTERING_FIRST);
                if (int rc = transform(sh, st, sh->khat, j1, l1))
                    return rc;
                if (int rc = means(sh, st, nullptr, first + 2 * a, first + 2 * a + 1))
                    return rc;
                if (j1 + 1 < J)
                    if (int rc = slicer_fft_forward_hypot(sh->fft, st, sh->X, sh->Y, sh->uhat))
                        return rc;
            }
            if (j1 + 1 == J)
                continue;
            ProfScope ps(h, KN_SCATTERING_SECOND);
            for (int j2 = j1 + 1; j2 < J; j2++)
                for (int l2 = 0; l2 < L; l2++) {
                    if (int rc = transform(sh, st, sh->uhat, j2, l2))
                        return rc;
                    if (int rc = means(sh, st, nullptr, second + a * JL + (size_t)j2 * L + l2, nullptr))
                        return rc;
                }
        }
    sh->ran = true;
    return SLICER_OK;
}

int slicer_scattering_read(slicer_scattering_handle sh, double *s0, double *s1, double *p1, double *s2)
{
    if (!sh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_scattering_read: null handle");
    if (!sh->ran)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_scattering_read before any slicer_scattering_run");
    std::vector<double> r(sh->res_count());
    if (int rc = sub_read(*sh, r.data(), sh->res, r.size() * sizeof(double)))
        return rc;
    const int J = sh->J, L = sh->L, JL = J * L;
    if (s0) {
        s0[0] = r[0];
        s0[1] = r[1];
    }
    for (int a = 0; a < JL; a++) {
        if (s1)
            s1[a] = r[2 + 2 * (size_t)a];
        if (p1)
            p1[a] = r[2 + 2 * (size_t)a + 1];
        if (s2)
            for (int b = 0; b < JL; b++)
                s2[(size_t)a * JL + b] = b / L > a / L ? r[2 + 2 * (size_t)JL + (size_t)a * JL + b] : (double)NAN;
    }
    return SLICER_OK;
}

int slicer_scattering_modulus(slicer_scattering_handle sh, const float *d_map, int32_t j1, int32_t l1, int32_t j2,
                              int32_t l2, double *host)
{
    const char *who = "slicer_scattering_modulus";
    if (!sh || !d_map || !host)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    slicer_handle h = sh->h;
    const int J = sh->J, L = sh->L;
    if (j1 < 0 || j1 >= J || l1 < 0 || l1 >= L)
        return fail(h, SLICER_ERR_ARG, "%s: (j1, l1) = (%d, %d) outside 0..%d, 0..%d", who, j1, l1, J - 1, L - 1);
    const bool order2 = !(j2 == -1 && l2 == -1);
    if (order2 && (j2 <= j1 || j2 >= J || l2 < 0 || l2 >= L))
        return fail(h, SLICER_ERR_ARG, "%s: (j2, l2) = (%d, %d) is neither (-1, -1) nor j1 < j2 <= %d, 0 <= l2 <= %d", who,
                    j2, l2, J - 1, L - 1);
    hipStream_t st;
    if (int rc = sub_stream(h, sh->device, &st))
        return rc;
    if (int rc = slicer_fft_forward(sh->fft, st, d_map, sh->khat))
        return rc;
    if (int rc = transform(sh, st, sh->khat, j1, l1))
        return rc;
    if (order2) {
        if (int rc = slicer_fft_forward_hypot(sh->fft, st, sh->X, sh->Y, sh->uhat))
            return rc;
        if (int rc = transform(sh, st, sh->uhat, j2, l2))
            return rc;
    }
    const size_t n2 = (size_t)sh->n * sh->n;
    hipLaunchKernelGGL(k_scat_modulus, dim3(groups_for(n2, 16, h->num_cus)), dim3(kThreads), 0, st, sh->X, sh->Y, n2);
    HIPCHK(h, hipGetLastError());
    return sub_read(*sh, host, sh->X, n2 * sizeof(double));
}

int slicer_scattering_destroy(slicer_scattering_handle sh) { return sub_destroy(sh); }
