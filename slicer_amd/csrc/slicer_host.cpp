// slicer_host.cpp -- what every file under the C ABI shares (slicer_host.hpp): the error text, grow-only device
// buffers, the per-kernel profile, and the helpers of the sub-handles (kappa, shear, FFT plan, power, moments, peaks, rays, smooth, noise, minkowski, bispectrum, starlet, l1norm, betti, scattering, catalogue).
#include "slicer_host.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "slicer_fft.hpp"

namespace {

thread_local std::string g_null_err;

const char *kKernelNames[] = {"direct_deposit", "finalize_tsc", "fold_ngp",  "synth",         "project_bin",
                              "bin_scan",       "bin_scatter",  "tile_deposit", "debug_project", "bin_sort",
                              "power_fft",      "power_bin",    "moments_sum", "moments",       "peaks",
                              "peaks_finish",   "rays_step",    "rays_observe", "smooth_rows",  "smooth_norm",
                              "smooth_cols",    "noise_add",    "noise_words",  "minkowski",    "minkowski_finish",
                              "bispectrum_fft", "bispectrum_band", "bispectrum", "bispectrum_finish",
                              "starlet_first",  "starlet_level", "starlet_last", "l1norm",       "l1norm_finish",
                              "betti_rank",     "betti_link",   "betti_finish", "scattering_first", "scattering_second"};
static_assert(sizeof kKernelNames / sizeof *kKernelNames == KN_COUNT, "one name per KN_* value");

}  // namespace

hipEvent_t get_event(slicer_handle h)
{
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess)
        return nullptr;  // ProfScope then skips timing for this launch
    return e;
}

int fail(slicer_handle h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h)
        h->err = buf;
    else
        g_null_err = buf;
    return code;
}

int ensure(slicer_handle h, DevBuf &b, size_t bytes, bool *fresh)
{
    if (fresh)
        *fresh = false;
    if (b.cap >= bytes)
        return SLICER_OK;
    if (b.p)
        HIPCHK(h, hipFree(b.p));  // implicit device synchronisation: happens only while a workspace still grows
    b.p = nullptr;
    b.cap = 0;
    HIPCHK(h, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    if (fresh)
        *fresh = true;
    return SLICER_OK;
}

void release(DevBuf &b)
{
    if (b.p)
        (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

ProfScope::ProfScope(slicer_handle h_, int name_) : h(h_), name(name_)
{
    if (h->profiling) {
        e0 = get_event(h);
        e1 = get_event(h);
        if (!e0 || !e1) {  // hipEventCreate failed: leave this launch untimed rather than record on a null event
            if (e0)
                h->ev_pool.push_back(e0);
            if (e1)
                h->ev_pool.push_back(e1);
            e0 = e1 = nullptr;
            h->prof_event_failures++;
        } else {
            (void)hipEventRecord(e0, h->stream);
        }
    }
}

ProfScope::~ProfScope()
{
    if (e0 && e1) {
        (void)hipEventRecord(e1, h->stream);
        h->prof.push_back({name, e0, e1});
    }
}

void prof_collect(slicer_handle h)
{
    for (auto &p : h->prof) {
        (void)hipEventSynchronize(p.e1);
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
            h->prof_ms[p.name] += ms;
            h->prof_n[p.name] += 1;
        }
        h->ev_pool.push_back(p.e0);
        h->ev_pool.push_back(p.e1);
    }
    h->prof.clear();
}

int sub_open(slicer_handle h, const char *who, hipStream_t *st, int *device)
{
    *st = h->stream;
    *device = 0;
    if (hipStreamGetDevice(*st, device) != hipSuccess)
        return fail(h, SLICER_ERR_HIP, "%s: the handle's stream has no device", who);
    if (hipSetDevice(*device) != hipSuccess)
        return fail(h, SLICER_ERR_HIP, "hipSetDevice(%d) failed", *device);
    return SLICER_OK;
}

int sub_stream(slicer_handle h, int device, hipStream_t *st)
{
    *st = h->stream;
    HIPCHK(h, hipSetDevice(device));
    return SLICER_OK;
}

int npix_in_range(slicer_handle h, const char *who, int npix, int max_npix)
{
    if (npix < 1)
        return fail(h, SLICER_ERR_ARG, "%s: npix must be positive", who);
    if (npix > max_npix)
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: npix = %d above %d", who, npix, max_npix);
    return SLICER_OK;
}

int sub_read(const SubHandle &s, void *host, const void *dev, size_t bytes)
{
    hipStream_t st;
    if (int rc = sub_stream(s.h, s.device, &st))
        return rc;
    HIPCHK(s.h, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(s.h, hipStreamSynchronize(st));
    return SLICER_OK;
}

int DevAllocs::alloc(int rc, slicer_handle h, const char *who, void **p, size_t bytes, const hipStream_t *zero_on)
{
    if (rc != SLICER_OK)
        return rc;
    hipError_t e = hipMalloc(p, bytes < 8 ? 8 : bytes);
    if (e != hipSuccess)
        return fail(h, e == hipErrorOutOfMemory ? SLICER_ERR_NOMEM : SLICER_ERR_HIP, "%s: %zu bytes of device memory: %s",
                    who, bytes, hipGetErrorString(e));
    ptrs.push_back(*p);
    if (zero_on && (e = hipMemsetAsync(*p, 0, bytes, *zero_on)) != hipSuccess)
        return fail(h, SLICER_ERR_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    return SLICER_OK;
}

void DevAllocs::replace(void *old, void *p)
{
    for (void *&q : ptrs)
        if (q == old)
            q = p;
}

void DevAllocs::free_all()
{
    for (void *p : ptrs)
        (void)hipFree(p);
    ptrs.clear();
}

bool fft_size_supported(int n)
{
    if (n < 2 || n > kFftMaxN)
        return false;
    for (int p : {2, 3, 5, 7})
        while (n % p == 0)
            n /= p;
    return n == 1;
}

extern "C" {

const char *slicer_last_error(slicer_handle h) { return h ? h->err.c_str() : g_null_err.c_str(); }

int slicer_profile_enable(slicer_handle h, int on)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!on && h->profiling)
        prof_collect(h);
    h->profiling = on != 0;
    return SLICER_OK;
}

int slicer_profile_reset(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    prof_collect(h);
    for (int i = 0; i < KN_COUNT; i++) {
        h->prof_ms[i] = 0;
        h->prof_n[i] = 0;
    }
    return SLICER_OK;
}

int slicer_profile_get(slicer_handle h, slicer_kernel_time *out, int capacity, int *n_out)
{
    if (!h || !n_out)
        return fail(h, SLICER_ERR_ARG, "null argument");
    prof_collect(h);
    int k = 0;
    for (int i = 0; i < KN_COUNT; i++) {
        if (!h->prof_n[i])
            continue;
        if (out && k < capacity) {
            memset(&out[k], 0, sizeof out[k]);
            strncpy(out[k].name, kKernelNames[i], sizeof(out[k].name) - 1);
            out[k].launches = h->prof_n[i];
            out[k].total_ms = h->prof_ms[i];
        }
        k++;
    }
    *n_out = k;
    return SLICER_OK;
}

}  // extern "C"
