// slicer_smooth.hip -- on-device Gaussian and aperture-mass smoothing of a map.
//
// Of an n x n f32 map x (row-major, only read), a scale s in pixels and a truncation t: R = floor(t s + 0.5) and the two
// f64 tables g_k = exp(-q_k), h_k = q_k g_k, q_k = k^2 / (2 s^2), k = 0 ... R (slicer_smooth_weights, host only).
// The line operator L_w along one axis, on f64 values v with samples outside the map taken as +0.0:
//   acc_0 = w_0 v[i];  acc_k = acc_{k-1} + w_k (v[i-k] + v[i+k]),  k = 1 ... R, from the centre outwards,
// every operation one IEEE f64 operation rounded once, no FMA (-ffp-contract=off).
//   SLICER_SMOOTH_GAUSS  T = L_g along axis 1, A = L_g of T along axis 0, N = L_g of a line of n ones,
//                        out[i][j] = (float)(A / (N[i] N[j])): renormalised by the weight that fell inside the map
//   SLICER_SMOOTH_MAP    G = L_g, H = L_h along axis 1, D = G - H, a = L_g of D, b = L_h of G along axis 0,
//                        out = (float)(c (a - b)), c = 1 / (2 pi s s): the aperture mass of U(r) = (1 - r^2 / 2 s^2)
//                        exp(-r^2 / 2 s^2) / (2 pi s^2); not renormalised
// The intermediates T (GAUSS) or D and G (MAP) are f64 in global memory owned by the handle, never rounded to f32.
//
// line4: what both kernels run.  A thread owns four adjacent outputs along the filtered axis and keeps the eight samples
// to the left of (and under) them and the eight to the right as f64 in registers.  Step k needs the windows moved by
// one sample each way, so four steps need one new block of four on each side: the loop is unrolled by four, every
// register index is static, and a step costs two fetched samples whatever R is.  The pair sum is shared between the
// g and the h chain; the four (MAP rows: eight) chains of a thread are independent.
//
// k_smooth_rows<KIND, VEC>: 256 threads take 4 rows x 256 columns, a wave one row segment, a lane four adjacent columns.
// The segment and a halo of R4 = 4 ceil(R / 4) <= 128 columns a side are staged as f32 in LDS (4 x 512 floats, the
// segment at window column 128, so every block of four is one 16-byte read on LDS's 16-byte grid).  Loads: a float4 per
// four pixels when 4 | n and the map is on the 16-byte grid (VEC), scalar loads otherwise; the window is the same.
// k_smooth_cols<KIND>: a tile of TH rows x TW columns of the f64 intermediate and R4 halo rows above and below it in
// LDS (dynamic: (TH + 2 R4) TW doubles, twice that for MAP's D and G); a thread takes one column and four adjacent
// rows, so a workgroup has TW TH / 4 threads (128 ... 1024): a tile that is alone on its CU still runs 2 waves a SIMD.
// TW (64 or 32) and TH (16 ... 64) come from the host (cols_cfg): the halo dominates at large R, so the tile that
// wastes least of a CU's 160 KiB is chosen per (kind, R).  The divisor N[i] N[j] or the constant c and the
// single rounding to f32 are fused into the store.  The order of every output's sum is fixed above, so the tile shapes
// change no bit.  k_smooth_norm fills N for the n of the run.  No atomics; nothing is carried over between runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxNpix = 131072;
constexpr int kMaxR = SLICER_SMOOTH_MAX_RADIUS;
constexpr int kPer = 4;                           // adjacent outputs of a thread along the filtered axis
constexpr int kRowsT0 = 4, kRowsT1 = 256;         // k_smooth_rows: tile rows x columns
constexpr int kHalo = 128;                        // ... window column of the tile's first pixel
constexpr int kPitch = kHalo + kRowsT1 + kHalo;   // ... floats of a window row
constexpr int kColsMaxThreads = 1024;             // k_smooth_cols: a thread per column and four rows of the tile
constexpr size_t kLdsOne = 156 * 1024;            // k_smooth_cols: the most one workgroup takes of a CU's 160 KiB; half of it leaves two on a CU

static_assert(kMaxR % kPer == 0 && kMaxR <= kHalo, "the halo holds the widest filter rounded up to whole blocks");
static_assert(kRowsT0 * kRowsT1 / kPer == kThreads, "one thread per four pixels of a row tile");
static_assert(64 * 64 / kPer <= kColsMaxThreads, "one thread per four pixels of the largest column tile");

// Four adjacent outputs of L_g (WG) and / or L_h (WH) of one line.  fetch(b, p) stores the four samples of block b at
// p[0 .. 3]: block 0 lies under the outputs, block -1 before it, block 1 after it, ...; blocks down to -ceil(R / 4) and
// up to ceil(R / 4) are fetched.  lw[i] is the sample 4 m + 4 - i before output 0 (i = 4 ... 7: those under the outputs
// shifted by 4 m), rw[i] the sample 4 m + i after it.
template <bool WG, bool WH, class Fetch>
__device__ __forceinline__ void line4(Fetch fetch, const double *__restrict__ g, const double *__restrict__ h, int R,
                                      double (&ag)[kPer], double (&ah)[kPer])
{
    double lw[2 * kPer], rw[2 * kPer];
    fetch(0, &lw[kPer]);
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        rw[q] = lw[kPer + q];
        if (WG)
            ag[q] = g[0] * rw[q];
        if (WH)
            ah[q] = h[0] * rw[q];
    }
    for (int m = 0; kPer * m < R; m++) {
        fetch(-(m + 1), &lw[0]);
        fetch(m + 1, &rw[kPer]);
        double wg4[kPer], wh4[kPer];  // (the tables are padded to whole blocks, so that the four loads are one)
#pragma unroll
        for (int s = 1; s <= kPer; s++) {
            wg4[s - 1] = WG ? g[kPer * m + s] : 0.0;
            wh4[s - 1] = WH ? h[kPer * m + s] : 0.0;
        }
#pragma unroll
        for (int s = 1; s <= kPer; s++) {
            const int k = kPer * m + s;
            if (k <= R) {  // (wave-uniform; the padding beyond R is never a factor)
                const double wg = wg4[s - 1], wh = wh4[s - 1];
#pragma unroll
                for (int q = 0; q < kPer; q++) {
                    const double pair = lw[kPer + q - s] + rw[q + s];
                    if (WG)
                        ag[q] = ag[q] + wg * pair;
                    if (WH)
                        ah[q] = ah[q] + wh * pair;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            lw[kPer + q] = lw[q];
            rw[q] = rw[kPer + q];
        }
    }
}

struct RowArgs {
    const float *x;
    const double *g, *h;  // [R4 + 1]: k = 0 ... R, then zeros that are loaded and never used
    double *mid;          // GAUSS: T [n][n]; MAP: D [n][n], then G [n][n]
    int n, R, R4;
    int tiles_x;
};

template <int KIND, bool VEC>
__global__ __launch_bounds__(kThreads) void k_smooth_rows(RowArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kRowsT0 * kPitch];
    const int n = a.n, R4 = a.R4, tid = threadIdx.x;
    const int wr = tid / 64, lane = tid % 64;  // a wave stages and filters one row of the tile
    const int r = (int)(blockIdx.x / (unsigned)a.tiles_x) * kRowsT0 + wr;
    const int c0 = (int)(blockIdx.x % (unsigned)a.tiles_x) * kRowsT1;
    float *row = win + wr * kPitch;
    const float *src = a.x + (size_t)(r < n ? r : 0) * n;
    // window columns kHalo - R4 ... kHalo + kRowsT1 + R4 - 1 = map columns c0 - R4 ... c0 + kRowsT1 + R4 - 1
    if (VEC) {  // 4 | n, 4 | c0, 4 | R4: a float4 lies in the map whole or not at all
        for (int q = lane; q < (kRowsT1 + 2 * R4) / kPer; q += 64) {
            const int wc = kHalo - R4 + kPer * q, c = c0 - kHalo + wc;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r < n && c >= 0 && c < n)
                v = *reinterpret_cast<const float4 *>(src + c);
            *reinterpret_cast<float4 *>(row + wc) = v;
        }
    } else {
        for (int q = lane; q < kRowsT1 + 2 * R4; q += 64) {
            const int wc = kHalo - R4 + q, c = c0 - kHalo + wc;
            row[wc] = r < n && c >= 0 && c < n ? src[c] : 0.0f;
        }
    }
    __syncthreads();
    const int j0 = c0 + kPer * lane;
    if (r >= n || j0 >= n)
        return;
    const float *centre = row + kHalo + kPer * lane;
    const auto fetch = [centre](int b, double *p) {
        const float4 v = *reinterpret_cast<const float4 *>(centre + kPer * b);
        p[0] = (double)v.x, p[1] = (double)v.y, p[2] = (double)v.z, p[3] = (double)v.w;
    };
    double ag[kPer], ah[kPer];
    line4<true, KIND == SLICER_SMOOTH_MAP>(fetch, a.g, a.h, a.R, ag, ah);
    const size_t at = (size_t)r * n + j0;
    double *first = a.mid + at;  // T, or D
    if (KIND == SLICER_SMOOTH_MAP) {
#pragma unroll
        for (int q = 0; q < kPer; q++)
            ah[q] = ag[q] - ah[q];  // D = G - H
    }
    const double *one = KIND == SLICER_SMOOTH_MAP ? ah : ag;
    if (VEC) {
        reinterpret_cast<double2 *>(first)[0] = make_double2(one[0], one[1]);
        reinterpret_cast<double2 *>(first)[1] = make_double2(one[2], one[3]);
        if (KIND == SLICER_SMOOTH_MAP) {
            double *second = first + (size_t)n * n;
            reinterpret_cast<double2 *>(second)[0] = make_double2(ag[0], ag[1]);
            reinterpret_cast<double2 *>(second)[1] = make_double2(ag[2], ag[3]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            if (j0 + q < n) {
                first[q] = one[q];
                if (KIND == SLICER_SMOOTH_MAP)
                    first[(size_t)n * n + q] = ag[q];
            }
        }
    }
}

// N[i] = L_g of a line of n ones: the weight of the filter that lies inside the map about sample i
__global__ __launch_bounds__(kThreads) void k_smooth_norm(const double *__restrict__ g, int n, int R, double *norm)
{
    const int i = (int)(blockIdx.x * (unsigned)kThreads + threadIdx.x);
    if (i >= n)
        return;
    double acc = g[0] * 1.0;
    for (int k = 1; k <= R; k++) {
        const double pair = (i - k >= 0 ? 1.0 : 0.0) + (i + k < n ? 1.0 : 0.0);
        acc = acc + g[k] * pair;
    }
    norm[i] = acc;
}

struct ColArgs {
    const double *mid;
    const double *g, *h;
    const double *norm;  // GAUSS: N [n]
    double c;            // MAP
    float *out;
    int n, R, R4;
    int tw_log2, th;     // the tile: 1 << tw_log2 columns x th rows, 16 | th
    int tiles_x;
};

template <int KIND>
__global__ __launch_bounds__(kColsMaxThreads) void k_smooth_cols(ColArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double tile[];
    constexpr int kPlanes = KIND == SLICER_SMOOTH_MAP ? 2 : 1;
    const int n = a.n, R4 = a.R4, tid = threadIdx.x;
    const int tw = 1 << a.tw_log2, wrows = a.th + 2 * R4;
    const int r0 = (int)(blockIdx.x / (unsigned)a.tiles_x) * a.th;
    const int c0 = (int)(blockIdx.x % (unsigned)a.tiles_x) << a.tw_log2;
    // window row wr = map row r0 - R4 + wr
    for (int q = tid; q < wrows << a.tw_log2; q += (int)blockDim.x) {
        const int wr = q >> a.tw_log2, wc = q & (tw - 1);
        const int r = r0 - R4 + wr, c = c0 + wc;
        const bool in = r >= 0 && r < n && c < n;
        const size_t at = in ? (size_t)r * n + c : 0;
#pragma unroll
        for (int p = 0; p < kPlanes; p++)
            tile[(size_t)p * (wrows << a.tw_log2) + q] = in ? a.mid[(size_t)p * n * n + at] : 0.0;
    }
    __syncthreads();
    const int wc = tid & (tw - 1), col = c0 + wc;
    if (col >= n)
        return;
    for (int rg = tid >> a.tw_log2; kPer * rg < a.th; rg += (int)blockDim.x >> a.tw_log2) {  // (once: cols_threads)
        const int i0 = r0 + kPer * rg;
        if (i0 >= n)
            break;
        const double *centre = tile + ((size_t)(R4 + kPer * rg) << a.tw_log2) + wc;
        const int tw_log2 = a.tw_log2;
        const auto fetch = [centre, tw_log2](int b, double *p) {
#pragma unroll
            for (int q = 0; q < kPer; q++)
                p[q] = centre[(kPer * b + q) * (1 << tw_log2)];
        };
        double ag[kPer], ah[kPer], unused[kPer];
        line4<true, false>(fetch, a.g, a.h, a.R, ag, unused);  // GAUSS: A of T; MAP: a of D
        if (KIND == SLICER_SMOOTH_MAP) {
            const double *centre_g = centre + (size_t)(wrows << a.tw_log2);
            const auto fetch_g = [centre_g, tw_log2](int b, double *p) {
#pragma unroll
                for (int q = 0; q < kPer; q++)
                    p[q] = centre_g[(kPer * b + q) * (1 << tw_log2)];
            };
            line4<false, true>(fetch_g, a.g, a.h, a.R, unused, ah);  // b of G
        }
        const double nj = KIND == SLICER_SMOOTH_GAUSS ? a.norm[col] : 0.0;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int i = i0 + q;
            if (i >= n)
                break;
            double v;
            if (KIND == SLICER_SMOOTH_GAUSS)
                v = ag[q] / (a.norm[i] * nj);
            else
                v = a.c * (ag[q] - ah[q]);
            a.out[(size_t)i * n + col] = (float)v;
        }
    }
}

struct ColsCfg {
    int tw_log2 = 0, th = 0;
    size_t lds = 0;
};

// The tile of k_smooth_cols for a kind and R4: of the tiles of 64 or 32 columns and 16 ... 64 rows that fit into half
// of kLdsOne (two workgroups on a CU) or into all of it, the one with the largest useful share th / (th + 2 R4) of its
// window, a lone workgroup counted at 0.8 and a half-width tile at 0.9 of that.  There always is one: the narrow tile
// of 2 x 32 doubles a row has 312 rows in kLdsOne, and 2 R4 <= 256.
ColsCfg cols_cfg(int kind, int R4)
{
    const size_t planes = kind == SLICER_SMOOTH_MAP ? 2 : 1;
    ColsCfg best;
    double best_score = 0.0;
    for (int lone = 0; lone < 2; lone++)
        for (int tw_log2 = 6; tw_log2 >= 5; tw_log2--) {
            const size_t row_bytes = (planes * sizeof(double)) << tw_log2;
            const int rows = (int)((lone ? kLdsOne : kLdsOne / 2) / row_bytes) - 2 * R4;
            const int th = std::min(64, rows / 16 * 16);
            if (th < 16)
                continue;
            const double score = (double)th / (th + 2 * R4) * (lone ? 0.8 : 1.0) * (tw_log2 == 6 ? 1.0 : 0.9);
            if (score > best_score) {
                best_score = score;
                best.tw_log2 = tw_log2;
                best.th = th;
                best.lds = (size_t)(th + 2 * R4) * row_bytes;
            }
        }
    return best;
}

// R, or the refusal.  `who` is the entry point for the message.
int radius_of(slicer_handle h, const char *who, double sigma_pix, double truncate, int *R)
{
    if (!std::isfinite(sigma_pix) || !(sigma_pix > 0))
        return fail(h, SLICER_ERR_ARG, "%s: sigma_pix must be positive and finite", who);
    if (!std::isfinite(truncate) || truncate < 1 || truncate > 8)
        return fail(h, SLICER_ERR_ARG, "%s: truncate must be within 1 ... 8", who);
    const double r = std::floor(truncate * sigma_pix + 0.5);  // scipy.ndimage.gaussian_filter's int(truncate * sd + 0.5)
    if (r < 1)
        return fail(h, SLICER_ERR_ARG, "%s: sigma_pix = %.17g, truncate = %.17g give the radius 0 (at least 1 pixel)", who,
                    sigma_pix, truncate);
    if (r > kMaxR)
        return fail(h, SLICER_ERR_UNSUPPORTED,
                    "%s: sigma_pix = %.17g, truncate = %.17g give a radius above %d pixels: run a wider filter on a level "
                    "of the moments pyramid (slicer_moments_device_map)",
                    who, sigma_pix, truncate, kMaxR);
    *R = (int)r;
    return SLICER_OK;
}

}  // namespace

struct slicer_smooth : SubHandle {
    int n = 0, kind = 0, R = 0;
    double c = 0.0;  // MAP: 1 / (2 pi s s)
    ColsCfg cols;
    std::vector<double> weights;  // g, then h, [R4 + 1] each: the tables, padded with zeros to whole blocks of steps
    double *d_weights = nullptr;
    double *mid = nullptr, *norm = nullptr;
    float *out = nullptr;
    int ran_n = 0;  // npix of the last run, 0 before any
};

extern "C" {

int slicer_smooth_weights(double sigma_pix, double truncate, int32_t *radius, double *g, double *h)
{
    int R = 0;
    if (int rc = radius_of(nullptr, "slicer_smooth_weights", sigma_pix, truncate, &R))
        return rc;
    if (radius)
        *radius = R;
    const double two_s2 = 2.0 * (sigma_pix * sigma_pix);
    for (int k = 0; k <= R; k++) {
        const double q = ((double)k * (double)k) / two_s2;
        const double gk = std::exp(-q);
        if (g)
            g[k] = gk;
        if (h)
            h[k] = q * gk;
    }
    return SLICER_OK;
}

int slicer_smooth_create(slicer_handle h, int32_t npix, int32_t kind, double sigma_pix, double truncate,
                         slicer_smooth_handle *out)
{
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    const char *who = "slicer_smooth_create";
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, who, npix, kMaxNpix))
        return rc;
    if (kind != SLICER_SMOOTH_GAUSS && kind != SLICER_SMOOTH_MAP)
        return fail(h, SLICER_ERR_ARG, "%s: kind = %d is neither SLICER_SMOOTH_GAUSS nor SLICER_SMOOTH_MAP", who, kind);
    int R = 0;
    if (int rc = radius_of(h, who, sigma_pix, truncate, &R))
        return rc;
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    hipStream_t st = nullptr;
    slicer_smooth_handle sh = nullptr;
    if (int rc = sub_new(h, who, &st, &sh))
        return rc;
    sh->n = npix;
    sh->kind = kind;
    sh->R = R;
    sh->c = 1.0 / (((2 * M_PI) * sigma_pix) * sigma_pix);
    const int R4 = (R + kPer - 1) / kPer * kPer;
    sh->cols = cols_cfg(kind, R4);
    sh->weights.assign(2 * (size_t)(R4 + 1), 0.0);
    int rc = slicer_smooth_weights(sigma_pix, truncate, nullptr, &sh->weights[0], &sh->weights[R4 + 1]);
    const size_t np2 = (size_t)npix * (size_t)npix, wbytes = sh->weights.size() * sizeof(double);
    if (rc == SLICER_OK) {
        const void *kern = kind == SLICER_SMOOTH_MAP ? (const void *)k_smooth_cols<SLICER_SMOOTH_MAP>
                                                     : (const void *)k_smooth_cols<SLICER_SMOOTH_GAUSS>;
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsOne) != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: cannot raise the LDS limit of the column kernel", who);
    }
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->d_weights, wbytes);
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->mid, (kind == SLICER_SMOOTH_MAP ? 2 : 1) * np2 * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->norm, (size_t)npix * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->out, np2 * sizeof(float));
    if (rc == SLICER_OK) {
        // (sh->weights outlives the copy)
        hipError_t e = hipMemcpyAsync(sh->d_weights, sh->weights.data(), wbytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: copying the weights: %s", who, hipGetErrorString(e));
    }
    return sub_done(rc, sh, out);
}

int slicer_smooth_run_npix(slicer_smooth_handle sh, const float *d_map, int32_t npix)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_smooth_run_npix: null argument");
    if (npix < 1 || npix > sh->n)
        return fail(sh->h, SLICER_ERR_ARG, "slicer_smooth_run_npix: npix = %d outside 1..%d", npix, sh->n);
    const size_t np2 = (size_t)npix * (size_t)npix;
    if (ranges_overlap(d_map, np2 * sizeof(float), sh->out, (size_t)sh->n * (size_t)sh->n * sizeof(float)))
        return fail(sh->h, SLICER_ERR_ARG, "slicer_smooth_run_npix: the input overlaps the handle's own output");
    hipStream_t st;
    if (int rc = sub_stream(sh->h, sh->device, &st))
        return rc;
    sh->ran_n = 0;
    const int R = sh->R, R4 = (R + kPer - 1) / kPer * kPer;
    const bool map = sh->kind == SLICER_SMOOTH_MAP;
    const double *g = sh->d_weights, *hh = sh->d_weights + (R4 + 1);
    {
        RowArgs a{};
        a.x = d_map;
        a.g = g;
        a.h = hh;
        a.mid = sh->mid;
        a.n = npix;
        a.R = R;
        a.R4 = R4;
        a.tiles_x = (npix + kRowsT1 - 1) / kRowsT1;
        const dim3 grid((unsigned)(a.tiles_x * ((npix + kRowsT0 - 1) / kRowsT0))), block(kThreads);
        const bool vec = npix % 4 == 0 && (uintptr_t)d_map % 16 == 0;
        ProfScope ps(sh->h, KN_SMOOTH_ROWS);
        if (map && vec)
            hipLaunchKernelGGL((k_smooth_rows<SLICER_SMOOTH_MAP, true>), grid, block, 0, st, a);
        else if (map)
            hipLaunchKernelGGL((k_smooth_rows<SLICER_SMOOTH_MAP, false>), grid, block, 0, st, a);
        else if (vec)
            hipLaunchKernelGGL((k_smooth_rows<SLICER_SMOOTH_GAUSS, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_smooth_rows<SLICER_SMOOTH_GAUSS, false>), grid, block, 0, st, a);
        HIPCHK(sh->h, hipGetLastError());
    }
    if (!map) {
        ProfScope ps(sh->h, KN_SMOOTH_NORM);
        hipLaunchKernelGGL(k_smooth_norm, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g, npix,
                           R, sh->norm);
        HIPCHK(sh->h, hipGetLastError());
    }
    {
        ColArgs a{};
        a.mid = sh->mid;
        a.g = g;
        a.h = hh;
        a.norm = sh->norm;
        a.c = sh->c;
        a.out = sh->out;
        a.n = npix;
        a.R = R;
        a.R4 = R4;
        a.tw_log2 = sh->cols.tw_log2;
        a.th = sh->cols.th;
        a.tiles_x = (npix + (1 << a.tw_log2) - 1) >> a.tw_log2;
        const dim3 grid((unsigned)(a.tiles_x * ((npix + a.th - 1) / a.th))), block((unsigned)((a.th / kPer) << a.tw_log2));
        ProfScope ps(sh->h, KN_SMOOTH_COLS);
        if (map)
            hipLaunchKernelGGL(k_smooth_cols<SLICER_SMOOTH_MAP>, grid, block, sh->cols.lds, st, a);
        else
            hipLaunchKernelGGL(k_smooth_cols<SLICER_SMOOTH_GAUSS>, grid, block, sh->cols.lds, st, a);
        HIPCHK(sh->h, hipGetLastError());
    }
    sh->ran_n = npix;
    return SLICER_OK;
}

int slicer_smooth_run(slicer_smooth_handle sh, const float *d_map)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_smooth_run: null argument");
    return slicer_smooth_run_npix(sh, d_map, sh->n);
}

int slicer_smooth_device_map(slicer_smooth_handle sh, float **d_out)
{
    if (!sh || !d_out)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_smooth_device_map: null argument");
    if (!sh->ran_n)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_smooth_device_map before any slicer_smooth_run");
    *d_out = sh->out;
    return SLICER_OK;
}

int slicer_smooth_read(slicer_smooth_handle sh, float *out)
{
    if (!sh || !out)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_smooth_read: null argument");
    if (!sh->ran_n)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_smooth_read before any slicer_smooth_run");
    return sub_read(*sh, out, sh->out, (size_t)sh->ran_n * (size_t)sh->ran_n * sizeof(float));
}

int slicer_smooth_destroy(slicer_smooth_handle sh) { return sub_destroy(sh); }

}  // extern "C"
