// slicer_lensing.hip -- on-device Born convergence maps (weights: slicer_lensing_host.cpp).
//
// kappa_s = sum_p c_sp (m_p - mean m_p) over the finalized total maps m_p of every plane, accumulated where the maps
// already are.  Per slicer_kappa_add (one pass: up to SLICER_MAX_PLANES maps), on the handle's stream:
//   k_kappa_add     every map read once (f32 x 4 per lane); for up to 8 sources per launch A_s += sum_p c_sp m_p in
//                   f64 (f64 x 2 accumulator accesses); the first launch of a batch also writes each workgroup's f64 sum
//                   of every map to `partials` (no float atomics).  More sources: more launches over the same maps.
//   k_kappa_means   one workgroup: the partials of each map summed in a fixed order -> mean_p; and, per group of 8
//                   sources, off_s += sum_p c_sp mean_p (the deferred mean subtraction).
// slicer_kappa_finalize: k_kappa_finalize writes (float)(A_s - off_s).  Every reduction has a fixed order and no
// kernel hands work across workgroups, so the same call sequence gives bitwise the same maps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_host.hpp"

namespace {

constexpr int kMaxMaps = SLICER_MAX_PLANES;
constexpr int kGroup = 8;       // sources per launch
constexpr int kThreads = 256;   // 4 waves; every lane owns 4 consecutive pixels

struct AddArgs {
    const float *maps[kMaxMaps];
    double *acc[kGroup];
    double c[kMaxMaps][kGroup];
    double *partials;  // [kMaxMaps][gridDim.x]
    uint64_t n;        // pixels per map
    int n_maps;
    unsigned active;   // bit j: source j of the group has a non-zero coefficient in this batch
    int write_partials;
};

struct MeansArgs {
    const double *partials;
    double *means;     // the batch's first map's slot
    double *off;       // the group's first source
    double c[kMaxMaps][kGroup];
    uint64_t n;
    unsigned nblocks;
    int n_maps;
    unsigned active;
    int compute_means;  // 1: the batch's means from the partials; 0: read them back (a later source group)
};

struct FinalizeArgs {
    const double *acc[kGroup];
    const double *off;
    float *out[kGroup];
    uint64_t n;
    int n_src;
};

__device__ inline double wave_sum(double x)  // fixed butterfly order: deterministic
{
    for (int m = 32; m >= 1; m >>= 1)
        x += __shfl_xor(x, m, 64);
    return x;
}

// VEC: every map pointer is 16-byte aligned (hipMalloc'd maps are); otherwise scalar loads
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_kappa_add(AddArgs a)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    const bool full = i0 + 4 <= a.n;
    const int cnt = i0 >= a.n ? 0 : (full ? 4 : (int)(a.n - i0));
    float m[kMaxMaps][4];
#pragma unroll
    for (int p = 0; p < kMaxMaps; p++) {
        m[p][0] = m[p][1] = m[p][2] = m[p][3] = 0.0f;
        if (p < a.n_maps) {
            if (VEC && full) {
                const float4 v = *reinterpret_cast<const float4 *>(a.maps[p] + i0);
                m[p][0] = v.x;
                m[p][1] = v.y;
                m[p][2] = v.z;
                m[p][3] = v.w;
            } else {
                for (int k = 0; k < cnt; k++)
                    m[p][k] = a.maps[p][i0 + k];
            }
        }
    }
#pragma unroll
    for (int s = 0; s < kGroup; s++) {
        if (!((a.active >> s) & 1u) || cnt == 0)
            continue;
        double add[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            double t = 0.0;
#pragma unroll
            for (int p = 0; p < kMaxMaps; p++)
                if (p < a.n_maps)
                    t += a.c[p][s] * (double)m[p][k];
            add[k] = t;
        }
        double *acc = a.acc[s] + i0;
        if (full) {
            double2 *q = reinterpret_cast<double2 *>(acc);
            double2 lo = q[0], hi = q[1];
            lo.x += add[0];
            lo.y += add[1];
            hi.x += add[2];
            hi.y += add[3];
            q[0] = lo;
            q[1] = hi;
        } else {
            for (int k = 0; k < cnt; k++)
                acc[k] += add[k];
        }
    }
    if (!a.write_partials)
        return;  // uniform over the launch
    __shared__ double red[kThreads / 64][kMaxMaps];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
    for (int p = 0; p < kMaxMaps; p++) {
        if (p < a.n_maps) {
            const double x = wave_sum(((double)m[p][0] + (double)m[p][1]) + ((double)m[p][2] + (double)m[p][3]));
            if (lane == 0)
                red[wave][p] = x;
        }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)a.n_maps) {
        const int p = threadIdx.x;
        a.partials[(size_t)p * gridDim.x + blockIdx.x] = (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]);
    }
}

__global__ __launch_bounds__(kThreads) void k_kappa_means(MeansArgs a)
{
    __shared__ double red[kThreads];
    __shared__ double mean[kMaxMaps];
    for (int p = 0; p < a.n_maps; p++) {
        if (a.compute_means) {
            double x = 0.0;
            for (unsigned b = threadIdx.x; b < a.nblocks; b += kThreads)
                x += a.partials[(size_t)p * a.nblocks + b];
            red[threadIdx.x] = x;
            __syncthreads();
            for (int w = kThreads / 2; w >= 1; w >>= 1) {
                if (threadIdx.x < (unsigned)w)
                    red[threadIdx.x] += red[threadIdx.x + w];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                mean[p] = red[0] / (double)a.n;
                a.means[p] = mean[p];
            }
            __syncthreads();
        } else if (threadIdx.x == 0) {
            mean[p] = a.means[p];
        }
    }
    __syncthreads();
    const int s = threadIdx.x;
    if (s < kGroup && ((a.active >> s) & 1u)) {
        double t = 0.0;
        for (int p = 0; p < a.n_maps; p++)
            t += a.c[p][s] * mean[p];
        a.off[s] += t;
    }
}

// accumulators and results are the library's own hipMalloc'd buffers: always 16-byte aligned
__global__ __launch_bounds__(kThreads) void k_kappa_finalize(FinalizeArgs a)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i0 >= a.n)
        return;
    const bool full = i0 + 4 <= a.n;
    for (int s = 0; s < a.n_src; s++) {
        const double off = a.off[s];
        const double *acc = a.acc[s] + i0;
        float *out = a.out[s] + i0;
        if (full) {
            const double2 lo = reinterpret_cast<const double2 *>(acc)[0], hi = reinterpret_cast<const double2 *>(acc)[1];
            *reinterpret_cast<float4 *>(out) =
                make_float4((float)(lo.x - off), (float)(lo.y - off), (float)(hi.x - off), (float)(hi.y - off));
        } else {
            for (uint64_t k = 0; k < a.n - i0 && k < 4; k++)
                out[k] = (float)(acc[k] - off);
        }
    }
}

}  // namespace

struct slicer_kappa_s : SubHandle {
    int npix = 0;
    uint64_t n = 0;
    int n_sources = 0;
    unsigned nblocks = 0;
    std::vector<double *> acc;   // [n_sources] f64 accumulators A_s
    std::vector<float *> kappa;  // [n_sources] f32 results
    double *off = nullptr;       // [n_sources] sum_p c_sp mean_p
    double *partials = nullptr;  // [kMaxMaps][nblocks]
    double *means = nullptr;     // [means_cap]
    int means_cap = 0;
    int n_added = 0;
    bool finalized = false;
};

int slicer_kappa_create(slicer_handle h, int32_t npix, int32_t n_sources, slicer_kappa_handle *out)
{
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_kappa_create: null argument");
    *out = nullptr;
    if (npix <= 0 || n_sources <= 0)
        return fail(h, SLICER_ERR_ARG, "slicer_kappa_create: npix and n_sources must be positive");
    const char *who = "slicer_kappa_create";
    hipStream_t st = nullptr;
    slicer_kappa_handle kh = nullptr;
    if (int rc = sub_new(h, who, &st, &kh))
        return rc;
    kh->npix = npix;
    kh->n = (uint64_t)npix * (uint64_t)npix;
    kh->n_sources = n_sources;
    kh->nblocks = (unsigned)((kh->n + 4ull * kThreads - 1) / (4ull * kThreads));
    int rc = SLICER_OK;
    kh->acc.assign(n_sources, nullptr);
    kh->kappa.assign(n_sources, nullptr);
    for (int s = 0; s < n_sources; s++) {
        rc = kh->mem.alloc(rc, h, who, (void **)&kh->acc[s], kh->n * sizeof(double), &st);
        rc = kh->mem.alloc(rc, h, who, (void **)&kh->kappa[s], kh->n * sizeof(float), &st);
    }
    rc = kh->mem.alloc(rc, h, who, (void **)&kh->off, n_sources * sizeof(double), &st);
    rc = kh->mem.alloc(rc, h, who, (void **)&kh->partials, (size_t)kMaxMaps * kh->nblocks * sizeof(double), &st);
    kh->means_cap = 1024;
    rc = kh->mem.alloc(rc, h, who, (void **)&kh->means, kh->means_cap * sizeof(double), &st);
    return sub_done(rc, kh, out);
}

int slicer_kappa_add(slicer_kappa_handle kh, int32_t n_maps, const float *const *d_maps, const double *coeff)
{
    if (!kh || !d_maps || !coeff)
        return fail(kh ? kh->h : nullptr, SLICER_ERR_ARG, "slicer_kappa_add: null argument");
    if (n_maps < 1 || n_maps > kMaxMaps)
        return fail(kh->h, SLICER_ERR_ARG, "slicer_kappa_add: n_maps = %d, expected 1..%d", n_maps, kMaxMaps);
    bool aligned = true;
    for (int p = 0; p < n_maps; p++) {
        if (!d_maps[p])
            return fail(kh->h, SLICER_ERR_ARG, "slicer_kappa_add: map %d is null", p);
        aligned = aligned && ((uintptr_t)d_maps[p] % 16) == 0;
    }
    hipStream_t st;
    if (int rc = sub_stream(kh->h, kh->device, &st))
        return rc;
    if (kh->n_added + n_maps > kh->means_cap) {  // rare: grow the means array (the copy is ordered on the stream)
        const int cap = std::max(2 * kh->means_cap, kh->n_added + n_maps);
        double *p = nullptr;
        HIPCHK(kh->h, hipMalloc(&p, cap * sizeof(double)));
        HIPCHK(kh->h, hipMemcpyAsync(p, kh->means, kh->n_added * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(kh->h, hipStreamSynchronize(st));
        HIPCHK(kh->h, hipFree(kh->means));
        kh->mem.replace(kh->means, p);
        kh->means = p;
        kh->means_cap = cap;
    }
    const int S = kh->n_sources;
    for (int g = 0; g * kGroup < S; g++) {
        const int ns = std::min(kGroup, S - g * kGroup);
        AddArgs a{};
        MeansArgs m{};
        for (int p = 0; p < n_maps; p++)
            a.maps[p] = d_maps[p];
        for (int j = 0; j < ns; j++) {
            a.acc[j] = kh->acc[g * kGroup + j];
            for (int p = 0; p < n_maps; p++) {
                const double c = coeff[(size_t)p * S + g * kGroup + j];
                a.c[p][j] = m.c[p][j] = c;
                if (c != 0.0)
                    a.active |= 1u << j;
            }
        }
        a.partials = kh->partials;
        a.n = kh->n;
        a.n_maps = n_maps;
        a.write_partials = g == 0;
        m.active = a.active;
        if (a.active || a.write_partials) {
            if (aligned)
                hipLaunchKernelGGL(k_kappa_add<true>, dim3(kh->nblocks), dim3(kThreads), 0, st, a);
            else
                hipLaunchKernelGGL(k_kappa_add<false>, dim3(kh->nblocks), dim3(kThreads), 0, st, a);
            HIPCHK(kh->h, hipGetLastError());
        }
        if (a.active || g == 0) {
            m.partials = kh->partials;
            m.means = kh->means + kh->n_added;
            m.off = kh->off + g * kGroup;
            m.n = kh->n;
            m.nblocks = kh->nblocks;
            m.n_maps = n_maps;
            m.compute_means = g == 0;
            hipLaunchKernelGGL(k_kappa_means, dim3(1), dim3(kThreads), 0, st, m);
            HIPCHK(kh->h, hipGetLastError());
        }
    }
    kh->n_added += n_maps;
    kh->finalized = false;
    return SLICER_OK;
}

int slicer_kappa_reset(slicer_kappa_handle kh)
{
    if (!kh)
        return fail(nullptr, SLICER_ERR_ARG, "null kappa handle");
    hipStream_t st;
    if (int rc = sub_stream(kh->h, kh->device, &st))
        return rc;
    // what slicer_kappa_create clears, and no more than is ever read before it is written: the accumulators and the offsets
    for (int s = 0; s < kh->n_sources; s++)
        HIPCHK(kh->h, hipMemsetAsync(kh->acc[s], 0, kh->n * sizeof(double), st));
    HIPCHK(kh->h, hipMemsetAsync(kh->off, 0, kh->n_sources * sizeof(double), st));
    kh->n_added = 0;
    kh->finalized = false;
    return SLICER_OK;
}

int slicer_kappa_plane_means(slicer_kappa_handle kh, double *out, int32_t max)
{
    if (!kh || (!out && max > 0))
        return fail(kh ? kh->h : nullptr, SLICER_ERR_ARG, "slicer_kappa_plane_means: null argument");
    hipStream_t st;
    if (int rc = sub_stream(kh->h, kh->device, &st))
        return rc;
    const int k = std::min<int>(std::max<int>(max, 0), kh->n_added);
    if (k > 0)
        HIPCHK(kh->h, hipMemcpyAsync(out, kh->means, k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(kh->h, hipStreamSynchronize(st));
    return SLICER_OK;
}

int slicer_kappa_finalize(slicer_kappa_handle kh)
{
    if (!kh)
        return fail(kh ? kh->h : nullptr, SLICER_ERR_ARG, "null kappa handle");
    hipStream_t st;
    if (int rc = sub_stream(kh->h, kh->device, &st))
        return rc;
    const int S = kh->n_sources;
    for (int g = 0; g * kGroup < S; g++) {
        FinalizeArgs f{};
        f.n_src = std::min(kGroup, S - g * kGroup);
        for (int j = 0; j < f.n_src; j++) {
            f.acc[j] = kh->acc[g * kGroup + j];
            f.out[j] = kh->kappa[g * kGroup + j];
        }
        f.off = kh->off + g * kGroup;
        f.n = kh->n;
        hipLaunchKernelGGL(k_kappa_finalize, dim3(kh->nblocks), dim3(kThreads), 0, st, f);
        HIPCHK(kh->h, hipGetLastError());
    }
    kh->finalized = true;
    return SLICER_OK;
}

int slicer_kappa_device_map(slicer_kappa_handle kh, int32_t s, float **d_map)
{
    if (!kh || !d_map)
        return fail(kh ? kh->h : nullptr, SLICER_ERR_ARG, "slicer_kappa_device_map: null argument");
    if (s < 0 || s >= kh->n_sources)
        return fail(kh->h, SLICER_ERR_ARG, "source %d out of range (%d sources)", s, kh->n_sources);
    if (!kh->finalized)
        return fail(kh->h, SLICER_ERR_STATE, "kappa maps are available after slicer_kappa_finalize");
    *d_map = kh->kappa[s];
    return SLICER_OK;
}

int slicer_kappa_read(slicer_kappa_handle kh, int32_t s, float *host)
{
    float *d = nullptr;
    if (int rc = slicer_kappa_device_map(kh, s, &d))
        return rc;
    if (!host)
        return fail(kh->h, SLICER_ERR_ARG, "slicer_kappa_read: null host pointer");
    return sub_read(*kh, host, d, kh->n * sizeof(float));
}

int slicer_kappa_destroy(slicer_kappa_handle kh) { return sub_destroy(kh); }
