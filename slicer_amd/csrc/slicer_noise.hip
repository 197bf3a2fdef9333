// slicer_noise.hip -- on-device shape noise for a map, counter-based.
//
// A map is a flat array of f32 pixels p = i npix + j; block b holds the pixels 4 b ... 4 b + 3 and draws once from
// Philox4x32-10 (slicer_philox.hpp): counter (lo b, hi b, realisation, stream), key (lo seed, hi seed) -> words w0 ... w3.
//   u(w) = (w + 0.5) 2^-32 (exact in f64, inside (0, 1));  R_a = sqrt(-2 log u(w0)),  R_b = sqrt(-2 log u(w2));
//   z0 = R_a cospi(2 u(w1)), z1 = R_a sinpi(2 u(w1)), z2 = R_b cospi(2 u(w3)), z3 = R_b sinpi(2 u(w3)),  all in f64;
//   out[p] = (float)((double)x[p] + sigma z)  (x == NULL: (float)(sigma z)), every operation rounded once, no FMA.
// So a pixel's value depends on (seed, stream, realisation, p) and on nothing else: not on the launch shape, the load
// path, the piece of the map a run covers or the map's size.
//
// k_noise_add<HAS_X, VEC>: a thread per block (grid-stride beyond 2^20 workgroups of 256): one Philox call, two logs, two
// square roots, two sincospi, four outputs.  VEC: x and the output are on the 16-byte grid, so a whole block is one float4
// load and one float4 store; otherwise, and for the last block of a run that ends inside it, scalar loads and stores of the
// same values.  x may be the output itself (a second layer): a thread reads its block before it writes it and touches no
// other.  No LDS, no atomics, no scratch.  k_noise_words: the raw words of a run of blocks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "slicer_host.hpp"
#include "slicer_philox.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxNpix = 131072;
constexpr uint64_t kMaxGroups = 1u << 20;  // workgroups of a launch; beyond them the threads stride

struct NoiseArgs {
    const float *x;  // [count], or null
    float *out;      // [count]
    uint64_t first_block, count;  // pixels 4 first_block ... 4 first_block + count - 1
    uint64_t seed;
    double sigma;
    uint32_t stream, realisation;
};

// the four normals of the words w
__device__ __forceinline__ void normals4(const uint32_t (&w)[4], double (&z)[4])
{
    const double ua = ((double)w[0] + 0.5) * 0x1p-32, ub = ((double)w[2] + 0.5) * 0x1p-32;
    const double ta = ((double)w[1] + 0.5) * 0x1p-31, tb = ((double)w[3] + 0.5) * 0x1p-31;  // 2 u, exact
    const double ra = sqrt(-2.0 * log(ua)), rb = sqrt(-2.0 * log(ub));
    double sa, ca, sb, cb;
    sincospi(ta, &sa, &ca);
    sincospi(tb, &sb, &cb);
    z[0] = ra * ca;
    z[1] = ra * sa;
    z[2] = rb * cb;
    z[3] = rb * sb;
}

template <bool HAS_X, bool VEC>
__global__ __launch_bounds__(kThreads) void k_noise_add(NoiseArgs a)
{
    const uint64_t n_blocks = (a.count + 3) / 4, stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < n_blocks; t += stride) {
        uint32_t w[4];
        slicer::noise_block_words(a.seed, a.stream, a.realisation, a.first_block + t, w);
        double z[4];
        normals4(w, z);
        const uint64_t at = 4 * t;
        const bool whole = at + 4 <= a.count;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (HAS_X) {
            if (VEC && whole) {
                const float4 q = *reinterpret_cast<const float4 *>(a.x + at);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (at + k < a.count)
                        v[k] = a.x[at + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double n = a.sigma * z[k];
            v[k] = HAS_X ? (float)((double)v[k] + n) : (float)n;
        }
        if (VEC && whole) {
            *reinterpret_cast<float4 *>(a.out + at) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (at + k < a.count)
                    a.out[at + k] = v[k];
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_noise_words(uint64_t seed, uint32_t stream, uint32_t realisation,
                                                          uint64_t first_block, uint64_t n_blocks, uint32_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < n_blocks; t += stride) {
        uint32_t w[4];
        slicer::noise_block_words(seed, stream, realisation, first_block + t, w);
#pragma unroll
        for (int k = 0; k < 4; k++)
            out[4 * t + k] = w[k];
    }
}

unsigned groups_of(uint64_t n_blocks) { return (unsigned)std::min<uint64_t>((n_blocks + kThreads - 1) / kThreads, kMaxGroups); }

int sigma_ok(slicer_handle h, const char *who, double sigma)
{
    if (!std::isfinite(sigma) || sigma < 0)
        return fail(h, SLICER_ERR_ARG, "%s: sigma must be finite and not negative", who);
    return SLICER_OK;
}

}  // namespace

struct slicer_noise : SubHandle {
    int n = 0;
    uint64_t seed = 0;
    float *out = nullptr;
    uint64_t ran = 0;  // pixels of the last run, 0 before any
};

extern "C" {

int slicer_noise_create(slicer_handle h, int32_t npix, uint64_t seed, slicer_noise_handle *out)
{
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    const char *who = "slicer_noise_create";
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, who, npix, kMaxNpix))
        return rc;
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    hipStream_t st = nullptr;
    slicer_noise_handle nh = nullptr;
    if (int rc = sub_new(h, who, &st, &nh))
        return rc;
    nh->n = npix;
    nh->seed = seed;
    const int rc = nh->mem.alloc(SLICER_OK, h, who, (void **)&nh->out, (size_t)npix * (size_t)npix * sizeof(float));
    return sub_done(rc, nh, out);
}

int slicer_noise_run_at(slicer_noise_handle nh, const float *d_map, uint64_t first_pixel, uint64_t count, double sigma,
                        uint32_t stream, uint32_t realisation)
{
    const char *who = "slicer_noise_run_at";
    slicer_handle h = nh ? nh->h : nullptr;
    if (int rc = sigma_ok(h, who, sigma))
        return rc;
    if (first_pixel % 4 != 0)
        return fail(h, SLICER_ERR_ARG, "%s: first_pixel must be a multiple of 4 (a run starts at a block)", who);
    if (!nh)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    const uint64_t np2 = (uint64_t)nh->n * (uint64_t)nh->n;
    if (count < 1 || count > np2)
        return fail(h, SLICER_ERR_ARG, "%s: count = %llu outside 1..%llu", who, (unsigned long long)count,
                    (unsigned long long)np2);
    // the output itself is a second layer; any other overlap is refused
    if (d_map && d_map != nh->out && ranges_overlap(d_map, count * sizeof(float), nh->out, np2 * sizeof(float)))
        return fail(h, SLICER_ERR_ARG, "%s: the input overlaps the handle's own output at another offset", who);
    hipStream_t st;
    if (int rc = sub_stream(h, nh->device, &st))
        return rc;
    nh->ran = 0;
    NoiseArgs a{};
    a.x = d_map;
    a.out = nh->out;
    a.first_block = first_pixel / 4;
    a.count = count;
    a.seed = nh->seed;
    a.sigma = sigma;
    a.stream = stream;
    a.realisation = realisation;
    const dim3 grid(groups_of((count + 3) / 4)), block(kThreads);
    const bool vec = ((uintptr_t)d_map | (uintptr_t)nh->out) % 16 == 0;
    {
        ProfScope ps(h, KN_NOISE_ADD);
        if (d_map && vec)
            hipLaunchKernelGGL((k_noise_add<true, true>), grid, block, 0, st, a);
        else if (d_map)
            hipLaunchKernelGGL((k_noise_add<true, false>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((k_noise_add<false, true>), grid, block, 0, st, a);
        HIPCHK(h, hipGetLastError());
    }
    nh->ran = count;
    return SLICER_OK;
}

int slicer_noise_run_npix(slicer_noise_handle nh, const float *d_map, int32_t npix, double sigma, uint32_t stream,
                          uint32_t realisation)
{
    const char *who = "slicer_noise_run_npix";
    slicer_handle h = nh ? nh->h : nullptr;
    if (int rc = sigma_ok(h, who, sigma))
        return rc;
    if (!nh)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    if (npix < 1 || npix > nh->n)
        return fail(h, SLICER_ERR_ARG, "%s: npix = %d outside 1..%d", who, npix, nh->n);
    return slicer_noise_run_at(nh, d_map, 0, (uint64_t)npix * (uint64_t)npix, sigma, stream, realisation);
}

int slicer_noise_run(slicer_noise_handle nh, const float *d_map, double sigma, uint32_t stream, uint32_t realisation)
{
    const char *who = "slicer_noise_run";
    if (int rc = sigma_ok(nh ? nh->h : nullptr, who, sigma))
        return rc;
    if (!nh)
        return fail(nullptr, SLICER_ERR_ARG, "%s: null argument", who);
    return slicer_noise_run_npix(nh, d_map, nh->n, sigma, stream, realisation);
}

int slicer_noise_words_device(slicer_noise_handle nh, uint64_t first_block, uint64_t n_blocks, uint32_t stream,
                              uint32_t realisation, uint32_t *d_out)
{
    const char *who = "slicer_noise_words_device";
    slicer_handle h = nh ? nh->h : nullptr;
    if (n_blocks < 1 || n_blocks > ((uint64_t)1 << 32))
        return fail(h, SLICER_ERR_ARG, "%s: n_blocks outside 1..2^32", who);
    if (!nh || !d_out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    hipStream_t st;
    if (int rc = sub_stream(h, nh->device, &st))
        return rc;
    ProfScope ps(h, KN_NOISE_WORDS);
    hipLaunchKernelGGL(k_noise_words, dim3(groups_of(n_blocks)), dim3(kThreads), 0, st, nh->seed, stream, realisation,
                       first_block, n_blocks, d_out);
    HIPCHK(h, hipGetLastError());
    return SLICER_OK;
}

int slicer_noise_device_map(slicer_noise_handle nh, float **d_out)
{
    if (!nh || !d_out)
        return fail(nh ? nh->h : nullptr, SLICER_ERR_ARG, "slicer_noise_device_map: null argument");
    if (!nh->ran)
        return fail(nh->h, SLICER_ERR_STATE, "slicer_noise_device_map before any slicer_noise_run");
    *d_out = nh->out;
    return SLICER_OK;
}

int slicer_noise_read(slicer_noise_handle nh, float *out)
{
    if (!nh || !out)
        return fail(nh ? nh->h : nullptr, SLICER_ERR_ARG, "slicer_noise_read: null argument");
    if (!nh->ran)
        return fail(nh->h, SLICER_ERR_STATE, "slicer_noise_read before any slicer_noise_run");
    return sub_read(*nh, out, nh->out, nh->ran * sizeof(float));
}

int slicer_noise_destroy(slicer_noise_handle nh) { return sub_destroy(nh); }

}  // extern "C"
