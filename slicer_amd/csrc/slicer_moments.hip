// slicer_moments.hip -- on-device central moments of a map over a pyramid of 2x2 halvings.
//
// Level 0 is the caller's n0 x n0 f32 map; level l+1 has n_{l+1} = n_l / 2 (integer division) pixels a side,
//   y[i][j] = ((x[2i][2j] + x[2i+1][2j]) + x[2i][2j+1]) + x[2i+1][2j+1]   in f32 (Lens/halve.py's order),
// stored as it is (SLICER_HALVE_SUM) or times 0.25f (SLICER_HALVE_MEAN).  Of every level the raw power sums
//   S_k = sum_i p_k(i),  d = (double)x_i - c,  p_2 = d * d,  p_k = p_{k-1} * d,  k = 2 ... 8,
// over ALL n_l^2 pixels about a centre c (the caller's, or the level's own mean), and the mean.
//
// One pass over level l (k_moments) reads it once, writes level l+1 and accumulates the seven sums of level l, the
// sum of the pixels it writes (the mean-to-be of level l+1) and, on request, the sum of the pixels it reads.  An
// *item* is two adjacent 2x2 blocks: rows 2i, 2i+1, columns 4q ... 4q+3 (one float4 of each row in, one float2 out),
// item t = i * Q + q with Q = ceil(h / 2), h = n / 2; for odd n the 2n-1 pixels of the last row and column follow as
// items of 8 pixels each.  Workgroup b takes items b * 2048 ... b * 2048 + 2047: thread tid takes item
// b * 2048 + j * 256 + tid for j = 0 ... 7, pixel after pixel in the order a0 a1 a2 a3 b0 b1 b2 b3 (row 2i, then row
// 2i+1).  Then the fixed wave butterfly of slicer_power.hip, an in-order sum over the four waves, one partial per
// workgroup and value; k_moments_finish (one workgroup per value) sums the partials: thread t takes partials t, t + 256,
// ... in order, then the same butterfly and wave sum.  It leaves the next level's mean in device memory, where the next
// pass reads its centre: no host round trip between the levels.  No atomics; the mapping does not depend on whether the
// pass stores (HALVE) or how it loads (VEC), so a level's sums are bitwise the same in a pyramid and alone.
//
// The mean of an m x m map is summed in the order in which a halving pass produces that map: items of two adjacent
// pixels of a row, t = i * ceil(m / 2) + q, eight items a thread.  k_moments does that for the levels it writes;
// k_moments_sum does it for level 0, reading the map instead of producing it.  The one exception is level 0 with its
// centre given (sumx): the map is read once, its mean is summed along with the S_k in their tree, and so it equals the
// mean of the other order within the mean's bound, not bitwise.  The S_k and the centres used are bitwise either way.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = 8;                           // items per thread
constexpr int64_t kGroupItems = kThreads * kItems;  // items per workgroup
constexpr int kOrders = SLICER_MOMENTS_ORDERS;
constexpr int kValues = kOrders + 2;  // S_2 ... S_8, the sum of the pixels read, the sum of the pixels written
constexpr int kSumX = kOrders, kSumY = kOrders + 1;
constexpr int kRes = 2 + kOrders;  // per level on the device: mean, centre used, S_2 ... S_8
constexpr int kMaxNpix = 131072;

// The geometry of one n x n level, host and device alike.
struct LevelGeom {
    int n, h, Q;
    int64_t T;     // items of 2x2 block pairs
    int64_t Tall;  // ... plus the items of the leftover row and column (odd n)
    int64_t G;     // workgroups of k_moments
    int64_t Ty;    // two-pixel items of the mean's tree
    int64_t Gy;    // workgroups that hold a partial of it
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

LevelGeom level_geom(int n)
{
    LevelGeom g{};
    g.n = n;
    g.h = n / 2;
    g.Q = (g.h + 1) / 2;
    g.T = (int64_t)g.h * g.Q;
    g.Tall = g.T + (n % 2 ? ceil_div(2 * (int64_t)n - 1, 8) : 0);
    g.G = ceil_div(g.Tall, kGroupItems);
    g.Ty = (int64_t)n * ((n + 1) / 2);
    g.Gy = ceil_div(g.Ty, kGroupItems);
    return g;
}

// f64 additions on the longest path of a tree of T items of `per` values each in G workgroups: the thread's own
// (every one counted, the first onto zero included), butterfly 6, waves 3; then the same over the partials.
int64_t tree_depth(int64_t T, int64_t G, int per)
{
    return per * std::min<int64_t>(kItems, ceil_div(T, kThreads)) + 9 + ceil_div(G, kThreads) + 9;
}

int64_t depth_of(int n)
{
    const LevelGeom g = level_geom(n);
    return std::max(tree_depth(g.Tall, g.G, 8), tree_depth(g.Ty, g.Gy, 2));
}

struct MomArgs {
    const float *x;
    float *y;             // level l+1 (HALVE)
    const double *c_dev;  // the level's own mean, read when c_given is NaN
    double c_given;
    double *partial;  // [kValues][pstride]
    size_t pstride;
    LevelGeom g;
    int mean_mode;  // HALVE: store 0.25f * y
    int sumx;       // also sum the pixels read
};

// The sum of v over the workgroup, in a fixed order; the result is valid in thread 0.
__device__ inline void wave_butterfly(double &v)
{
#pragma unroll
    for (int off = 32; off >= 1; off /= 2)
        v += __shfl_xor(v, off, 64);
}

template <bool HALVE, bool VEC>
__global__ __launch_bounds__(kThreads) void k_moments(MomArgs a)
{
    __shared__ double red[kWaves][kValues];
    const double c = isnan(a.c_given) ? *a.c_dev : a.c_given;
    const int n = a.g.n, h = a.g.h, Q = a.g.Q;
    const int tid = threadIdx.x;
    double s[kOrders];
#pragma unroll
    for (int k = 0; k < kOrders; k++)
        s[k] = 0.0;
    double sx = 0.0, sy = 0.0;
    const int64_t base = (int64_t)blockIdx.x * kGroupItems + tid;
#pragma unroll 2
    for (int j = 0; j < kItems; j++) {
        const int64_t t = base + (int64_t)j * kThreads;
        if (t >= a.g.Tall)
            break;
        float v[8];
        bool ok[8];
        if (t < a.g.T) {
            const int i = (int)(t / Q), q = (int)(t - (int64_t)i * Q);
            const size_t r0 = (size_t)(2 * i) * n + 4 * (size_t)q;
            if (VEC) {  // 4 | n: every pair is whole and on the 16-byte grid
                const float4 A = *reinterpret_cast<const float4 *>(a.x + r0);
                const float4 B = *reinterpret_cast<const float4 *>(a.x + r0 + n);
                v[0] = A.x, v[1] = A.y, v[2] = A.z, v[3] = A.w;
                v[4] = B.x, v[5] = B.y, v[6] = B.z, v[7] = B.w;
#pragma unroll
                for (int e = 0; e < 8; e++)
                    ok[e] = true;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const bool in = 4 * q + e < 2 * h;  // the second block of the last pair is missing for odd h
                    ok[e] = ok[4 + e] = in;
                    v[e] = in ? a.x[r0 + e] : 0.0f;
                    v[4 + e] = in ? a.x[r0 + n + e] : 0.0f;
                }
            }
            if (HALVE) {
                float y0 = ((v[0] + v[4]) + v[1]) + v[5], y1 = ((v[2] + v[6]) + v[3]) + v[7];
                if (a.mean_mode) {
                    y0 = 0.25f * y0;
                    y1 = 0.25f * y1;
                }
                const size_t o = (size_t)i * h + 2 * (size_t)q;
                if (VEC) {
                    *reinterpret_cast<float2 *>(a.y + o) = make_float2(y0, y1);
                } else {
                    a.y[o] = y0;
                    if (ok[2])
                        a.y[o + 1] = y1;
                }
                sy += (double)y0;
                if (ok[2])
                    sy += (double)y1;
            }
        } else {  // odd n: pixels 8u ... 8u+7 of the last row (n of them), then of the last column above it (n-1)
            const int64_t u = t - a.g.T;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int64_t p = 8 * u + e;
                ok[e] = p < 2 * (int64_t)n - 1;
                const size_t at = p < n ? (size_t)(n - 1) * n + (size_t)p : (size_t)(p - n) * n + (size_t)(n - 1);
                v[e] = ok[e] ? a.x[at] : 0.0f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            if (!ok[e])
                continue;
            const double xe = (double)v[e], d = xe - c;
            double p = d * d;
            s[0] += p;
#pragma unroll
            for (int k = 1; k < kOrders; k++) {
                p = p * d;
                s[k] += p;
            }
            if (a.sumx)
                sx += xe;
        }
    }

    const int lane = tid % 64, wave = tid / 64;
#pragma unroll
    for (int k = 0; k < kOrders; k++) {
        wave_butterfly(s[k]);
        if (lane == 0)
            red[wave][k] = s[k];
    }
    wave_butterfly(sx);
    wave_butterfly(sy);
    if (lane == 0) {
        red[wave][kSumX] = sx;
        red[wave][kSumY] = sy;
    }
    __syncthreads();
    if (tid < kValues) {
        double r = red[0][tid];
        for (int w = 1; w < kWaves; w++)
            r += red[w][tid];
        a.partial[(size_t)tid * a.pstride + blockIdx.x] = r;
    }
}

// The pixel sum of an m x m map in the order of the halving pass that would have written it (rows of kSumY).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_moments_sum(const float *x, int m, int64_t Ty, double *partial)
{
    __shared__ double red[kWaves];
    const int Qm = (m + 1) / 2, tid = threadIdx.x;
    double sy = 0.0;
    const int64_t base = (int64_t)blockIdx.x * kGroupItems + tid;
#pragma unroll 4
    for (int j = 0; j < kItems; j++) {
        const int64_t t = base + (int64_t)j * kThreads;
        if (t >= Ty)
            break;
        const int i = (int)(t / Qm), q = (int)(t - (int64_t)i * Qm);
        const size_t o = (size_t)i * m + 2 * (size_t)q;
        if (VEC) {  // even m on the 8-byte grid
            const float2 y = *reinterpret_cast<const float2 *>(x + o);
            sy += (double)y.x;
            sy += (double)y.y;
        } else {
            sy += (double)x[o];
            if (2 * q + 1 < m)
                sy += (double)x[o + 1];
        }
    }
    wave_butterfly(sy);
    if (tid % 64 == 0)
        red[tid / 64] = sy;
    __syncthreads();
    if (tid == 0) {
        double r = red[0];
        for (int w = 1; w < kWaves; w++)
            r += red[w];
        partial[blockIdx.x] = r;
    }
}

struct FinArgs {
    const double *partial;
    size_t pstride;
    int G, Gy;         // partials of S_k and of the pixels read; of the pixels written
    double *res;       // this level's kRes doubles (sums != 0)
    double *res_next;  // the level whose mean the written pixels give (Gy > 0)
    double c_given;
    double N, Nnext;
    int sums, sumx;
};

// Workgroup v sums the partials of value v in workgroup order and puts the result where it belongs.
__global__ __launch_bounds__(kThreads) void k_moments_finish(FinArgs a)
{
    __shared__ double red[kWaves];
    const int v = blockIdx.x, tid = threadIdx.x;
    const bool active = v < kOrders ? a.sums != 0 : (v == kSumX ? a.sums && a.sumx : a.Gy > 0);
    if (!active)
        return;
    const int cnt = v == kSumY ? a.Gy : a.G;
    const double *p = a.partial + (size_t)v * a.pstride;
    double acc = 0.0;
#pragma unroll 8
    for (int k = tid; k < cnt; k += kThreads)
        acc += p[k];
    wave_butterfly(acc);
    if (tid % 64 == 0)
        red[tid / 64] = acc;
    __syncthreads();
    if (tid != 0)
        return;
    double r = red[0];
    for (int w = 1; w < kWaves; w++)
        r += red[w];
    if (v < kOrders) {
        a.res[2 + v] = r;
        if (v == 0)  // (with sumx the centre is given, so res[0], written by workgroup kSumX, is not read here)
            a.res[1] = isnan(a.c_given) ? a.res[0] : a.c_given;
    } else if (v == kSumX) {
        a.res[0] = r / a.N;
    } else {
        a.res_next[0] = r / a.Nnext;
    }
}

int floor_log2(int n)
{
    int l = 0;
    while (n >> (l + 1))
        l++;
    return l;
}

}  // namespace

struct slicer_moments : SubHandle {
    int n0 = 0, levels = 0, mode = 0;
    std::vector<LevelGeom> geom;  // levels + 1
    std::vector<float *> maps;    // [0] unused (the caller's), 1 ... levels
    double *partial = nullptr, *res = nullptr;
    size_t pstride = 0;
    bool ran = false;
};

extern "C" {

int slicer_moments_depth(int32_t npix)
{
    if (npix < 1 || npix > kMaxNpix) {
        fail(nullptr, SLICER_ERR_ARG, "slicer_moments_depth: npix = %d outside 1..%d", npix, kMaxNpix);
        return -1;
    }
    return (int)depth_of(npix);
}

int slicer_moments_create(slicer_handle h, int32_t npix, int32_t levels, int32_t mode, slicer_moments_handle *out)
{
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    const char *who = "slicer_moments_create";
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, who, npix, kMaxNpix))
        return rc;
    if (levels < 0 || levels > floor_log2(npix))
        return fail(h, SLICER_ERR_ARG, "slicer_moments_create: levels = %d outside 0..%d for npix = %d", levels,
                    floor_log2(npix), npix);
    if (mode != SLICER_HALVE_MEAN && mode != SLICER_HALVE_SUM)
        return fail(h, SLICER_ERR_ARG, "slicer_moments_create: mode = %d, expected SLICER_HALVE_MEAN or SLICER_HALVE_SUM",
                    mode);
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_moments_create: null argument");
    hipStream_t st = nullptr;
    slicer_moments_handle mh = nullptr;
    if (int rc = sub_new(h, who, &st, &mh))
        return rc;
    mh->n0 = npix;
    mh->levels = levels;
    mh->mode = mode;
    mh->maps.assign(levels + 1, nullptr);
    int rc = SLICER_OK;
    int64_t most = 1;
    for (int l = 0, n = npix; l <= levels; l++, n /= 2) {
        mh->geom.push_back(level_geom(n));
        most = std::max({most, mh->geom[l].G, mh->geom[l].Gy});
        if (l)
            rc = mh->mem.alloc(rc, h, who, (void **)&mh->maps[l], (size_t)n * n * sizeof(float));
    }
    mh->pstride = (size_t)most;
    rc = mh->mem.alloc(rc, h, who, (void **)&mh->partial, kValues * mh->pstride * sizeof(double));
    rc = mh->mem.alloc(rc, h, who, (void **)&mh->res, (size_t)(levels + 1) * kRes * sizeof(double));
    return sub_done(rc, mh, out);
}

int slicer_moments_run(slicer_moments_handle mh, const float *d_map, const double *centres)
{
    if (!mh || !d_map)
        return fail(mh ? mh->h : nullptr, SLICER_ERR_ARG, "slicer_moments_run: null argument");
    hipStream_t st;
    if (int rc = sub_stream(mh->h, mh->device, &st))
        return rc;
    mh->ran = false;
    const double c0 = centres ? centres[0] : (double)NAN;
    if (std::isnan(c0)) {  // level 0's own mean: a pass of its own
        ProfScope ps(mh->h, KN_MOMENTS_SUM);
        const LevelGeom &g = mh->geom[0];
        const bool vec = g.n % 2 == 0 && (uintptr_t)d_map % 8 == 0;
        double *part = mh->partial + (size_t)kSumY * mh->pstride;
        if (vec)
            hipLaunchKernelGGL(k_moments_sum<true>, dim3((unsigned)g.Gy), dim3(kThreads), 0, st, d_map, g.n, g.Ty, part);
        else
            hipLaunchKernelGGL(k_moments_sum<false>, dim3((unsigned)g.Gy), dim3(kThreads), 0, st, d_map, g.n, g.Ty, part);
        HIPCHK(mh->h, hipGetLastError());
        FinArgs f{};
        f.partial = mh->partial;
        f.pstride = mh->pstride;
        f.Gy = (int)g.Gy;
        f.res_next = mh->res;
        f.Nnext = (double)g.n * (double)g.n;
        hipLaunchKernelGGL(k_moments_finish, dim3(kValues), dim3(kThreads), 0, st, f);
        HIPCHK(mh->h, hipGetLastError());
    }
    ProfScope ps(mh->h, KN_MOMENTS);
    for (int l = 0; l <= mh->levels; l++) {
        const LevelGeom &g = mh->geom[l];
        const float *x = l ? mh->maps[l] : d_map;
        const bool halve = l < mh->levels;
        const bool vec = g.n % 4 == 0 && (uintptr_t)x % 16 == 0;
        MomArgs a{};
        a.x = x;
        a.y = halve ? mh->maps[l + 1] : nullptr;
        a.c_dev = mh->res + (size_t)l * kRes;
        a.c_given = centres ? centres[l] : (double)NAN;
        a.partial = mh->partial;
        a.pstride = mh->pstride;
        a.g = g;
        a.mean_mode = mh->mode == SLICER_HALVE_MEAN;
        a.sumx = l == 0 && !std::isnan(c0);  // a given centre: level 0's mean comes out of this pass
        const dim3 grid((unsigned)g.G), block(kThreads);
        if (halve && vec)
            hipLaunchKernelGGL((k_moments<true, true>), grid, block, 0, st, a);
        else if (halve)
            hipLaunchKernelGGL((k_moments<true, false>), grid, block, 0, st, a);
        else if (vec)
            hipLaunchKernelGGL((k_moments<false, true>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_moments<false, false>), grid, block, 0, st, a);
        HIPCHK(mh->h, hipGetLastError());
        FinArgs f{};
        f.partial = mh->partial;
        f.pstride = mh->pstride;
        f.G = (int)g.G;
        f.Gy = halve ? (int)mh->geom[l + 1].Gy : 0;
        f.res = mh->res + (size_t)l * kRes;
        f.res_next = halve ? mh->res + (size_t)(l + 1) * kRes : nullptr;
        f.c_given = a.c_given;
        f.N = (double)g.n * (double)g.n;
        f.Nnext = halve ? (double)mh->geom[l + 1].n * (double)mh->geom[l + 1].n : 1.0;
        f.sums = 1;
        f.sumx = a.sumx;
        hipLaunchKernelGGL(k_moments_finish, dim3(kValues), dim3(kThreads), 0, st, f);
        HIPCHK(mh->h, hipGetLastError());
    }
    mh->ran = true;
    return SLICER_OK;
}

int slicer_moments_read(slicer_moments_handle mh, int32_t *npix_level, double *means, double *centres_used, double *sums)
{
    if (!mh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_moments_read: null handle");
    if (!mh->ran)
        return fail(mh->h, SLICER_ERR_STATE, "slicer_moments_read before any slicer_moments_run");
    std::vector<double> r((size_t)(mh->levels + 1) * kRes);
    if (int rc = sub_read(*mh, r.data(), mh->res, r.size() * sizeof(double)))
        return rc;
    for (int l = 0; l <= mh->levels; l++) {
        if (npix_level)
            npix_level[l] = mh->geom[l].n;
        if (means)
            means[l] = r[(size_t)l * kRes];
        if (centres_used)
            centres_used[l] = r[(size_t)l * kRes + 1];
        if (sums)
            std::copy_n(&r[(size_t)l * kRes + 2], kOrders, sums + (size_t)l * kOrders);
    }
    return SLICER_OK;
}

int slicer_moments_device_map(slicer_moments_handle mh, int32_t level, float **d_map)
{
    if (!mh || !d_map)
        return fail(mh ? mh->h : nullptr, SLICER_ERR_ARG, "slicer_moments_device_map: null argument");
    *d_map = nullptr;
    if (level < 1 || level > mh->levels)
        return fail(mh->h, SLICER_ERR_ARG, "slicer_moments_device_map: level = %d outside 1..%d", level, mh->levels);
    if (!mh->ran)
        return fail(mh->h, SLICER_ERR_STATE, "slicer_moments_device_map before any slicer_moments_run");
    *d_map = mh->maps[level];
    return SLICER_OK;
}

int slicer_moments_read_map(slicer_moments_handle mh, int32_t level, float *host)
{
    if (!mh || !host)
        return fail(mh ? mh->h : nullptr, SLICER_ERR_ARG, "slicer_moments_read_map: null argument");
    float *d = nullptr;
    if (int rc = slicer_moments_device_map(mh, level, &d))
        return rc;
    const size_t n = (size_t)mh->geom[level].n;
    return sub_read(*mh, host, d, n * n * sizeof(float));
}

int slicer_moments_destroy(slicer_moments_handle mh) { return sub_destroy(mh); }

}  // extern "C"
