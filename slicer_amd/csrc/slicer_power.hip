// slicer_power.hip -- on-device binned auto and cross power spectra of kappa maps.
//
// For n_maps maps kappa_s, n x n f32 of side theta radians: khat_s = rfft2(kappa_s) in f64 on the [n][n/2+1] half
// plane (slicer_fft.hip, the transform shared with the shear handle).  Mode (i0, i1) has the integer radius^2 m2 = j0^2 + j1^2,
// j0 the signed fftfreq index of i0, j1 = i1; it is in bin b iff e2[b] <= m2 < e2[b+1] (e2 = the edges squared in f64;
// the last bin is closed on the right), and
//   C_st,b = theta^2 / n^4 * (1 / N_b) * sum over the bin's modes of Re(khat_s conj khat_t).
// N_b and the mean radius depend only on the geometry: slicer_power_bins computes them on the host.
//
// Binning: the modes of bin b in the row of |j0| = a form one contiguous j1 run (m2 grows with j1), found from a square
// root and an exact integer correction against the f64 edge squares (first_at_least).  The host cuts every bin into
// slices of rows a (about kSliceModes modes each).  k_power_bin: one workgroup per (slice, block pair of sources).  It
// walks its rows in chunks of kRowsPerChunk: the 2 runs of each row (+a and -a) go to LDS with a prefix sum of their
// lengths, and thread k takes modes k, k + kBinThreads, ... of the chunk.  A thread reads the spectra of its two source
// blocks once per mode and accumulates every pair of them in registers; a fixed wave butterfly and an in-order sum over
// the waves give one partial per (pair, slice).  k_power_finish sums a bin's slices in slice order.  No atomics: the
// summation order of every (pair, bin) is fixed by the geometry alone, so the results are bitwise repeatable and C_ss
// is the same whether it is computed alone (auto) or among all pairs (cross).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_power_internal.hpp"
#include "slicer_host.hpp"

namespace {

constexpr int kMaxMaps = 128;
constexpr int kBinThreads = 256;
constexpr int kWaves = kBinThreads / 64;
constexpr int kRowsPerChunk = kBinThreads / 2;  // two runs (+a, -a) per row value a
constexpr int kBlock = 8;                       // sources per block in cross mode
constexpr int64_t kSliceModes = 8192;          // target modes per workgroup slice of a bin

// Rows of |j0| = a: +a (i0 = a) exists for a <= (n-1)/2, -a (i0 = n - a) for 1 <= a <= n/2.
__host__ __device__ inline bool row_exists(int n, int a, int neg) { return neg ? a >= 1 && a <= n / 2 : a <= (n - 1) / 2; }

struct BinArgs {
    const double2 *spec;  // spectra of the sources, s at spec + s * stride
    size_t stride;
    const double *e2;    // edge squares, B + 1
    const int4 *slices;  // {bin, a0, a1, -}
    double *partial;     // [pair][nslices]
    int n, H, B, nslices;
    int S;          // sources in spec (cross); 1 (auto)
    int nblocks;    // ceil(S / BW)
    int pair_auto;  // auto mode: the pair (row of partial) of the one source; -1 in cross mode
};

__device__ inline int pair_index(int s, int t, int S) { return s * S - s * (s - 1) / 2 + (t - s); }

// RE (BW = 1, the pseudo-C_l handle's coupling matrix): the sum of the real parts instead of the squared moduli.
template <int BW, bool RE = false>
__global__ __launch_bounds__(kBinThreads) void k_power_bin(BinArgs a)
{
    __shared__ int run_row[kBinThreads], run_lo[kBinThreads], run_off[kBinThreads + 1];
    __shared__ double red[kWaves][BW * BW];
    const int4 sl = a.slices[blockIdx.x];
    // block pair (bi, bj), bi <= bj, in row-major order of the upper triangle
    int bi = 0, rem = blockIdx.y;
    while (rem >= a.nblocks - bi) {
        rem -= a.nblocks - bi;
        bi++;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int nsi = min(BW, a.S - bi * BW), nsj = min(BW, a.S - bj * BW);
    const double2 *pi = a.spec + (size_t)(bi * BW) * a.stride, *pj = a.spec + (size_t)(bj * BW) * a.stride;
    const int b = sl.x, tid = threadIdx.x;
    const double lo2 = a.e2[b], hi2 = a.e2[b + 1];
    const bool last = b == a.B - 1;

    double acc[BW][BW];
#pragma unroll
    for (int s = 0; s < BW; s++)
#pragma unroll
        for (int t = 0; t < BW; t++)
            acc[s][t] = 0.0;

    for (int c0 = sl.y; c0 < sl.z; c0 += kRowsPerChunk) {
        {
            const int ra = c0 + tid / 2, neg = tid & 1;
            int len = 0, lo = 0, row = 0;
            if (ra < sl.z && row_exists(a.n, ra, neg)) {
                const double a2 = (double)ra * (double)ra;
                lo = first_at_least(a2, lo2, false, a.H);
                const int hi = first_at_least(a2, hi2, last, a.H);
                len = max(hi - lo, 0);
                row = neg ? a.n - ra : ra;
            }
            run_row[tid] = row;
            run_lo[tid] = lo;
            run_off[tid + 1] = len;
            if (tid == 0)
                run_off[0] = 0;
        }
        __syncthreads();
        // inclusive scan of run_off[1..kBinThreads] (Hillis-Steele; integers, order-free)
        for (int d = 1; d < kBinThreads; d *= 2) {
            const int v = tid >= d ? run_off[tid + 1 - d] : 0;
            __syncthreads();
            run_off[tid + 1] += v;
            __syncthreads();
        }
        const int total = run_off[kBinThreads];
        for (int m = tid; m < total; m += kBinThreads) {
            int l = 0, h = kBinThreads;  // the run r with run_off[r] <= m < run_off[r + 1]
            while (h - l > 1) {
                const int mid = (l + h) / 2;
                if (run_off[mid] <= m)
                    l = mid;
                else
                    h = mid;
            }
            const size_t idx = (size_t)run_row[l] * a.H + (size_t)(run_lo[l] + m - run_off[l]);
            double2 x[BW], y[BW];
#pragma unroll
            for (int s = 0; s < BW; s++)
                x[s] = s < nsi ? pi[(size_t)s * a.stride + idx] : make_double2(0.0, 0.0);
#pragma unroll
            for (int t = 0; t < BW; t++)
                y[t] = diag ? x[t] : (t < nsj ? pj[(size_t)t * a.stride + idx] : make_double2(0.0, 0.0));
#pragma unroll
            for (int s = 0; s < BW; s++)
#pragma unroll
                for (int t = 0; t < BW; t++) {
                    const double p = RE ? x[s].x : x[s].x * y[t].x + x[s].y * y[t].y;
                    acc[s][t] += p;
                }
        }
        __syncthreads();  // the runs of this chunk are read by all threads before the next chunk overwrites them
    }

    const int lane = tid % 64, wave = tid / 64;
#pragma unroll
    for (int s = 0; s < BW; s++)
#pragma unroll
        for (int t = 0; t < BW; t++) {
            double v = acc[s][t];
#pragma unroll
            for (int off = 32; off >= 1; off /= 2)
                v += __shfl_xor(v, off, 64);
            if (lane == 0)
                red[wave][s * BW + t] = v;
        }
    __syncthreads();
    if (tid < BW * BW) {
        const int s = tid / BW, t = tid % BW;
        if (s < nsi && t < nsj && !(diag && t < s)) {
            double v = red[0][tid];
            for (int w = 1; w < kWaves; w++)
                v += red[w][tid];
            const int p = a.pair_auto >= 0 ? a.pair_auto : pair_index(bi * BW + s, bj * BW + t, a.S);
            a.partial[(size_t)(a.pair_auto >= 0 ? 0 : p) * a.nslices + blockIdx.x] = v;
        }
    }
}

// cl[pair0 + q][b] = norm * (sum of the partials of bin b's slices, in slice order) / N_b; NaN for an empty bin
__global__ void k_power_finish(const double *partial, const int *slice_off, const double *nmodes, double *cl,
                               int npairs, int B, int nslices, int pair0, double norm)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs * B)
        return;
    const int q = i / B, b = i % B;
    double sum = 0.0;
    for (int k = slice_off[b]; k < slice_off[b + 1]; k++)
        sum += partial[(size_t)q * nslices + k];
    cl[(size_t)(pair0 + q) * B + b] = nmodes[b] > 0.0 ? sum / nmodes[b] * norm : (double)NAN;
}

}  // namespace

// The edges, or 0 .. npix-1 for NULL (then n_edges must be npix); "" if they are usable, else why not (slicer_power_internal.hpp).
const char *check_edges(int npix, int n_edges, const double *edges, std::vector<double> &out)
{
    if (n_edges < 2)
        return "fewer than 2 edges";
    if (!edges) {
        if (n_edges != npix)
            return "n_edges must be npix for the default edges (edges = NULL)";
        out.resize(npix);
        for (int i = 0; i < npix; i++)
            out[i] = i;
        return "";
    }
    out.assign(edges, edges + n_edges);
    for (int i = 0; i < n_edges; i++) {
        if (!std::isfinite(out[i]) || out[i] < 0.0)
            return "edges must be finite and non-negative";
        if (i && !(out[i] > out[i - 1]))
            return "edges must be strictly ascending";
    }
    return "";
}

namespace {

// N_b and the sum of sqrt(m2) over every mode of the half plane (host; long double sums)
void bin_modes(int n, const std::vector<double> &edges, std::vector<int64_t> &counts, std::vector<double> &mean)
{
    const int B = (int)edges.size() - 1, H = n / 2 + 1;
    std::vector<double> e2(B + 1);
    for (int b = 0; b <= B; b++)
        e2[b] = edges[b] * edges[b];
    counts.assign(B, 0);
    std::vector<long double> sum(B, 0.0L);
    for (int a = 0; a <= n / 2; a++) {
        const int mult = (int)row_exists(n, a, 0) + (int)row_exists(n, a, 1);
        if (!mult)
            continue;
        const double a2 = (double)a * (double)a;
        int b = (int)(std::upper_bound(e2.begin(), e2.end(), a2) - e2.begin()) - 1;  // last edge <= m2
        for (int j = 0; j < H; j++) {
            const double m2 = a2 + (double)j * (double)j;
            while (b < B && e2[b + 1] <= m2)
                b++;
            int bin = b;
            if (b == B)
                bin = m2 == e2[B] ? B - 1 : -2;
            if (bin == -2)
                break;  // beyond the last edge, and so is the rest of the row
            if (bin < 0)
                continue;
            counts[bin] += mult;
            sum[bin] += (long double)mult * sqrtl((long double)m2);
        }
    }
    mean.assign(B, NAN);
    for (int b = 0; b < B; b++)
        if (counts[b])
            mean[b] = (double)(sum[b] / (long double)counts[b]);
}

}  // namespace

struct slicer_power_s : SubHandle {
    slicer_fft_s *fft = nullptr;
    int n = 0, H = 0, S = 0, cross = 0, B = 0, npairs = 0, nslices = 0;
    double ell_f = 0.0, norm = 0.0;
    std::vector<int64_t> counts;
    std::vector<double> mean_radius;
    double2 *spec = nullptr;  // n_maps (cross) or 1 (auto) spectra of n * H
    double *e2 = nullptr, *partial = nullptr, *nmodes = nullptr, *cl = nullptr;
    int4 *slices = nullptr;
    int *slice_off = nullptr;
    bool ran = false;
    SLICER_FFT_INTERNAL ~slicer_power_s() { slicer_fft_destroy(fft); }
};

namespace {

// Bin the spectra at ph->spec (S of them in cross mode, the one of source `s` in auto mode) into ph->cl.
int bin_launch(slicer_power_handle ph, hipStream_t st, int s)
{
    BinArgs a{};
    a.spec = ph->spec;
    a.stride = (size_t)ph->n * ph->H;
    a.e2 = ph->e2;
    a.slices = ph->slices;
    a.partial = ph->partial;
    a.n = ph->n;
    a.H = ph->H;
    a.B = ph->B;
    a.nslices = ph->nslices;
    int npairs;
    if (ph->cross) {
        a.S = ph->S;
        a.nblocks = (ph->S + kBlock - 1) / kBlock;
        a.pair_auto = -1;
        npairs = ph->npairs;
        const dim3 grid((unsigned)ph->nslices, (unsigned)(a.nblocks * (a.nblocks + 1) / 2));
        hipLaunchKernelGGL(k_power_bin<kBlock>, grid, dim3(kBinThreads), 0, st, a);
    } else {
        a.S = 1;
        a.nblocks = 1;
        a.pair_auto = s;
        npairs = 1;
        hipLaunchKernelGGL(k_power_bin<1>, dim3((unsigned)ph->nslices), dim3(kBinThreads), 0, st, a);
    }
    HIPCHK(ph->h, hipGetLastError());
    const int total = npairs * ph->B, tpb = 256;
    hipLaunchKernelGGL(k_power_finish, dim3((unsigned)((total + tpb - 1) / tpb)), dim3(tpb), 0, st, ph->partial,
                       ph->slice_off, ph->nmodes, ph->cl, npairs, ph->B, ph->nslices, ph->cross ? 0 : s, ph->norm);
    HIPCHK(ph->h, hipGetLastError());
    return SLICER_OK;
}

}  // namespace

int slicer_power_bins(int32_t npix, int32_t n_edges, const double *edges, int64_t *counts, double *mean_radius)
{
    if (npix < 1 || npix > 65536 || !counts || !mean_radius)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_power_bins: npix out of 1..65536, or null output");
    std::vector<double> e;
    const char *why = check_edges(npix, n_edges, edges, e);
    if (*why)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_power_bins: %s", why);
    std::vector<int64_t> c;
    std::vector<double> m;
    bin_modes(npix, e, c, m);
    std::copy(c.begin(), c.end(), counts);
    std::copy(m.begin(), m.end(), mean_radius);
    return SLICER_OK;
}

int slicer_power_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_maps, int32_t cross,
                        int32_t n_edges, const double *edges, slicer_power_handle *out)
{
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_power_create: null argument");
    *out = nullptr;
    if (!fft_size_supported(npix))
        return fail(h, SLICER_ERR_UNSUPPORTED,
                    "slicer_power_create: npix = %d unsupported (2..16384, prime factors 2, 3, 5, 7 only)", npix);
    if (n_maps < 1 || n_maps > kMaxMaps)
        return fail(h, SLICER_ERR_UNSUPPORTED, "slicer_power_create: n_maps = %d outside 1..%d", n_maps, kMaxMaps);
    if (cross != 0 && cross != 1)
        return fail(h, SLICER_ERR_ARG, "slicer_power_create: cross = %d, expected 0 or 1", cross);
    std::vector<double> e;
    const char *why = check_edges(npix, n_edges, edges, e);
    if (*why)
        return fail(h, SLICER_ERR_ARG, "slicer_power_create: %s", why);
    if (!std::isfinite(angle_deg) || angle_deg <= 0.0)
        return fail(h, SLICER_ERR_ARG, "slicer_power_create: the angle must be positive and finite");
    const char *who = "slicer_power_create";
    hipStream_t st = nullptr;
    slicer_power_handle ph = nullptr;
    if (int rc = sub_new(h, who, &st, &ph))
        return rc;
    const int n = npix, H = n / 2 + 1, B = n_edges - 1;
    ph->n = n;
    ph->H = H;
    ph->S = n_maps;
    ph->cross = cross;
    ph->B = B;
    ph->npairs = cross ? n_maps * (n_maps + 1) / 2 : n_maps;
    const double theta = angle_deg * M_PI / 180.0;
    ph->ell_f = 2.0 * M_PI / theta;
    ph->norm = theta * theta / ((double)n * (double)n * (double)n * (double)n);
    bin_modes(n, e, ph->counts, ph->mean_radius);

    // slices: bin b's rows a in [0, A_b), A_b = 1 + the largest a <= n/2 with a^2 <= e2[b+1], cut into ns_b equal
    // ranges of about kSliceModes modes; none for an empty bin
    std::vector<double> e2(B + 1), nm(B);
    for (int b = 0; b <= B; b++)
        e2[b] = e[b] * e[b];
    std::vector<int4> sl;
    std::vector<int> off(B + 1, 0);
    for (int b = 0; b < B; b++) {
        off[b] = (int)sl.size();
        nm[b] = (double)ph->counts[b];
        if (!ph->counts[b])
            continue;
        int amax = std::min(n / 2, (int)std::floor(std::sqrt(std::min(e2[b + 1], 1e18))));
        while (amax < n / 2 && (double)(amax + 1) * (amax + 1) <= e2[b + 1])
            amax++;
        while (amax > 0 && (double)amax * amax > e2[b + 1])
            amax--;
        const int64_t A = amax + 1;
        const int64_t ns = std::min(A, std::max<int64_t>(1, (ph->counts[b] + kSliceModes - 1) / kSliceModes));
        for (int64_t k = 0; k < ns; k++)
            sl.push_back(make_int4(b, (int)(A * k / ns), (int)(A * (k + 1) / ns), 0));
    }
    off[B] = (int)sl.size();
    ph->nslices = (int)sl.size();

    int rc = slicer_fft_create(h, n, h->opt.shear_split, st, ph->device, who, &ph->fft);
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->spec, (size_t)(cross ? n_maps : 1) * n * H * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->e2, (B + 1) * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->partial, (size_t)(cross ? ph->npairs : 1) * ph->nslices * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->nmodes, B * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->cl, (size_t)ph->npairs * B * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->slices, sl.size() * sizeof(int4));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->slice_off, (B + 1) * sizeof(int));
    auto up = [&](void *d, const void *hsrc, size_t bytes) {
        if (rc == SLICER_OK && bytes) {
            hipError_t err = hipMemcpyAsync(d, hsrc, bytes, hipMemcpyHostToDevice, st);
            if (err != hipSuccess)
                rc = fail(h, SLICER_ERR_HIP, "slicer_power_create: upload: %s", hipGetErrorString(err));
        }
    };
    up(ph->e2, e2.data(), (B + 1) * sizeof(double));
    up(ph->nmodes, nm.data(), B * sizeof(double));
    up(ph->slices, sl.data(), sl.size() * sizeof(int4));
    up(ph->slice_off, off.data(), (B + 1) * sizeof(int));
    if (rc == SLICER_OK && hipStreamSynchronize(st) != hipSuccess)  // the sources are host temporaries
        rc = fail(h, SLICER_ERR_HIP, "slicer_power_create: upload failed");
    return sub_done(rc, ph, out);
}

slicer_fft_s *slicer_power_plan(slicer_power_handle ph) { return ph->fft; }

int slicer_power_bin_real(slicer_power_handle ph, hipStream_t st, const double2 *spec, double norm, int column,
                          double *d_out)
{
    BinArgs a{};
    a.spec = spec;
    a.stride = (size_t)ph->n * ph->H;
    a.e2 = ph->e2;
    a.slices = ph->slices;
    a.partial = ph->partial;
    a.n = ph->n;
    a.H = ph->H;
    a.B = ph->B;
    a.nslices = ph->nslices;
    a.S = 1;
    a.nblocks = 1;
    a.pair_auto = 0;
    if (ph->nslices) {
        hipLaunchKernelGGL((k_power_bin<1, true>), dim3((unsigned)ph->nslices), dim3(kBinThreads), 0, st, a);
        HIPCHK(ph->h, hipGetLastError());
    }
    const int tpb = 256;
    hipLaunchKernelGGL(k_power_finish, dim3((unsigned)((ph->B + tpb - 1) / tpb)), dim3(tpb), 0, st, ph->partial,
                       ph->slice_off, ph->nmodes, d_out, 1, ph->B, ph->nslices, column, norm);
    HIPCHK(ph->h, hipGetLastError());
    return SLICER_OK;
}

int slicer_power_run(slicer_power_handle ph, const float *const *d_maps)
{
    if (!ph || !d_maps)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_power_run: null argument");
    for (int s = 0; s < ph->S; s++)
        if (!d_maps[s])
            return fail(ph->h, SLICER_ERR_ARG, "slicer_power_run: map %d is null", s);
    return slicer_power_run_masked(ph, d_maps, nullptr);
}

int slicer_power_run_masked(slicer_power_handle ph, const float *const *d_maps, const float *d_w)
{
    hipStream_t st;
    if (int rc = sub_stream(ph->h, ph->device, &st))
        return rc;
    const size_t stride = (size_t)ph->n * ph->H;
    auto forward = [&](int s) {
        ProfScope ps(ph->h, KN_POWER_FFT);
        double2 *khat = ph->spec + (ph->cross ? s * stride : 0);
        return d_w ? slicer_fft_forward_masked(ph->fft, st, d_maps[s], d_w, khat)
                   : slicer_fft_forward(ph->fft, st, d_maps[s], khat);
    };
    auto binning = [&](int s) {
        ProfScope ps(ph->h, KN_POWER_BIN);
        return bin_launch(ph, st, s);
    };
    ph->ran = false;
    if (ph->cross) {
        for (int s = 0; s < ph->S; s++)
            if (int rc = forward(s))
                return rc;
        if (int rc = binning(0))
            return rc;
    } else {
        for (int s = 0; s < ph->S; s++) {
            if (int rc = forward(s))
                return rc;
            if (int rc = binning(s))
                return rc;
        }
    }
    ph->ran = true;
    return SLICER_OK;
}

int slicer_power_transform_masked(slicer_power_handle ph, hipStream_t st, int s, const float *d_map, const float *d_w)
{
    ProfScope ps(ph->h, KN_POWER_FFT);
    ph->ran = false;
    return slicer_fft_forward_masked(ph->fft, st, d_map, d_w, slicer_power_stored(ph, s));
}

double2 *slicer_power_stored(slicer_power_handle ph, int s) { return ph->spec + (size_t)s * ph->n * ph->H; }

int slicer_power_bin_stored(slicer_power_handle ph, hipStream_t st, double *d_copy)
{
    {
        ProfScope ps(ph->h, KN_POWER_BIN);
        if (int rc = bin_launch(ph, st, 0))
            return rc;
    }
    if (d_copy)
        HIPCHK(ph->h, hipMemcpyAsync(d_copy, ph->cl, (size_t)ph->npairs * ph->B * sizeof(double),
                                     hipMemcpyDeviceToDevice, st));
    ph->ran = true;
    return SLICER_OK;
}

int slicer_power_spectrum(slicer_power_handle ph, int32_t map, double *host)
{
    if (!ph || !host)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_power_spectrum: null argument");
    if (map < 0 || map >= ph->S)
        return fail(ph->h, SLICER_ERR_ARG, "slicer_power_spectrum: map = %d outside 0..%d", map, ph->S - 1);
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_power_spectrum before any slicer_power_run");
    if (!ph->cross && map != ph->S - 1)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_power_spectrum: auto mode keeps only the last map's spectrum");
    const size_t stride = (size_t)ph->n * ph->H;
    return sub_read(*ph, host, ph->spec + (ph->cross ? map * stride : 0), stride * sizeof(double2));
}

int slicer_power_read(slicer_power_handle ph, double *cl, double *ell_mean, int64_t *counts)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_power_read: null handle");
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_power_read before any slicer_power_run");
    hipStream_t st;
    if (int rc = sub_stream(ph->h, ph->device, &st))
        return rc;
    if (cl)
        HIPCHK(ph->h, hipMemcpyAsync(cl, ph->cl, (size_t)ph->npairs * ph->B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ph->h, hipStreamSynchronize(st));
    for (int b = 0; b < ph->B; b++) {
        if (ell_mean)
            ell_mean[b] = ph->ell_f * ph->mean_radius[b];
        if (counts)
            counts[b] = ph->counts[b];
    }
    return SLICER_OK;
}

int slicer_power_destroy(slicer_power_handle ph) { return sub_destroy(ph); }
