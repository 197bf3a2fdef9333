// slicer_capi.cpp -- the C ABI of the core pass declared in include/slicer_amd.h: handle, options, stream, plane_*,
// file_*, deposit_*, plane_read and the device memory helpers; argument checks and host staging.  What they call lives
// next door (slicer_host.hpp lists the files).  Reference behaviour mirrored per entry point is cited in the header.
#include "slicer_host.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace slicer;

namespace {

int env_int(const char *name, int dflt = 0)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// Device -> host copy of a map into the caller's (pageable) array.  (Pinning the destination with hipHostRegister
// for the duration of the copy was measured on MI355X and bought nothing -- 8.5 ms per createDensityMaps call either
// way: registering 64 MiB costs what the direct DMA saves -- so the plain copy stays.)
int copy_map_to_host(slicer_handle h, void *dst, const void *d_src, size_t bytes)
{
    HIPCHK(h, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return SLICER_OK;
}

}  // namespace

int check_deposit_args(slicer_handle h, int type, const void *pos, const void *mass, uint64_t n)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane || !h->in_file)
        return fail(h, SLICER_ERR_STATE, "deposit outside slicer_plane_begin/slicer_file_begin");
    if (type < 0 || type > 5)
        return fail(h, SLICER_ERR_ARG, "particle type %d out of range 0..5", type);
    if (n && !pos)
        return fail(h, SLICER_ERR_ARG, "null position pointer with n = %llu", (unsigned long long)n);
    (void)mass;
    return SLICER_OK;
}

namespace {

int begin_type(slicer_handle h, int type, bool has_mass)
{
    const slicer_plane_desc &d = h->desc;
    int rc = prepare_type(h, type, has_mass);
    if (rc)
        return rc;
    if (d.mas == SLICER_MAS_NGP) {
        int mode = has_mass ? 2 : 1;
        if (h->file_mode[type] && h->file_mode[type] != mode)
            return fail(h, SLICER_ERR_ARG, "type %d deposited both with and without per-particle masses in one file",
                        type);
        h->file_mode[type] = mode;
        h->file_mconst[type] = (float)h->file.massarr[type];
        if (d.snopt > 0)  // kept entries carry (float)(pow(2, snopt) * m)   densitymaps.cpp:394
            h->file_mconst[type] = (float)(std::pow(2, d.snopt) * (double)(float)h->file.massarr[type]);
    }
    return SLICER_OK;
}

int ensure_staging(slicer_handle h, bool need_mass)
{
    uint64_t cap = h->max_chunk;
    if (h->stage_cap < cap) {
        for (int i = 0; i < 2; i++) {
            if (h->h_stage[i])
                (void)hipHostFree(h->h_stage[i]);
            if (h->d_stage[i])
                (void)hipFree(h->d_stage[i]);
            h->h_stage[i] = h->d_stage[i] = nullptr;
            if (h->h_mstage[i])
                (void)hipHostFree(h->h_mstage[i]);
            if (h->d_mstage[i])
                (void)hipFree(h->d_mstage[i]);
            h->h_mstage[i] = h->d_mstage[i] = nullptr;
            HIPCHK(h, hipHostMalloc((void **)&h->h_stage[i], cap * 12, hipHostMallocDefault));
            HIPCHK(h, hipMalloc((void **)&h->d_stage[i], cap * 12));
            if (!h->stage_free[i])
                HIPCHK(h, hipEventCreateWithFlags(&h->stage_free[i], hipEventDisableTiming));
        }
        h->stage_cap = cap;
    }
    if (need_mass && !h->h_mstage[0]) {
        for (int i = 0; i < 2; i++) {
            HIPCHK(h, hipHostMalloc((void **)&h->h_mstage[i], h->stage_cap * 4, hipHostMallocDefault));
            HIPCHK(h, hipMalloc((void **)&h->d_mstage[i], h->stage_cap * 4));
        }
    }
    return SLICER_OK;
}

}  // namespace

extern "C" {

int slicer_version(void) { return SLICER_AMD_VERSION; }

int slicer_create(int device, uint64_t max_chunk, slicer_handle *out)
{
    if (!out)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_create: out is null");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, SLICER_ERR_NO_DEVICE, "no HIP device available (%s)",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return fail(nullptr, SLICER_ERR_ARG, "device %d out of range (have %d)", device, ndev);
    slicer_handle h = new (std::nothrow) slicer_handle_s;
    if (!h)
        return fail(nullptr, SLICER_ERR_NOMEM, "out of host memory");
    h->device = device;
    for (const OptionName &o : kOptionNames)  // the environment seeds the knobs once; slicer_set_option changes them
        h->opt.*(o.field) = env_int(o.env, h->opt.*(o.field));
    // record cursors are 32-bit: one kernel pass carries at most 2^30 particles
    h->max_chunk = max_chunk ? std::min<uint64_t>(max_chunk, 1ull << 30) : (1ull << 24);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&h->own) != hipSuccess ||
        // one block: the selected-entry counters, the guard flag, the mass maxima (one memset per pass clears them)
        hipMalloc((void **)&h->d_counts, kPassScalarsBytes) != hipSuccess) {
        int rc = fail(nullptr, SLICER_ERR_HIP, "device %d initialisation failed: %s", device,
                      hipGetErrorString(hipGetLastError()));
        delete h;
        return rc;
    }
    h->d_neg = reinterpret_cast<int *>(h->d_counts + SLICER_MAX_PLANES * 6);
    h->d_maxmass = reinterpret_cast<unsigned *>(h->d_neg + 1);
    h->stream = h->own;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        h->num_cus = cus;
    *out = h;
    return SLICER_OK;
}

int slicer_destroy(slicer_handle h)
{
    if (!h)
        return SLICER_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    prof_collect(h);
    thin_drop(h);
    pass_stream_return(h);
    for (auto e : h->ev_pool)
        (void)hipEventDestroy(e);
    for (auto &pl : h->planes) {
        release(pl.tot);
        release(pl.acc_shared);
        for (int t = 0; t < 6; t++) {
            release(pl.toti[t]);
            release(pl.acc[t]);
        }
    }
    if (h->d_sweep)
        (void)hipFree(h->d_sweep);
    for (DevBuf *b : {&h->w_cxy, &h->w_cbin, &h->w_cm, &h->w_hist, &h->w_hist16, &h->w_total, &h->w_bcount, &h->w_items,
                      &h->w_tcounts, &h->w_tbase, &h->w_urand, &h->w_randtab, &h->w_randstate, &h->w_randwaves, &h->w_c1, &h->w_sboff, &h->w_sbstart, &h->w_sbn})
        release(*b);
    for (auto &Q : h->pg) {
        release(Q.w_tot);
        for (int i = 0; i < kMaxPending; i++) {
            release(Q.w_sxy[i]);
            release(Q.w_base[i]);
            release(Q.w_ptab[i]);
        }
    }
    for (int i = 0; i < 2; i++) {
        if (h->h_stage[i]) (void)hipHostFree(h->h_stage[i]);
        if (h->d_stage[i]) (void)hipFree(h->d_stage[i]);
        if (h->h_mstage[i]) (void)hipHostFree(h->h_mstage[i]);
        if (h->d_mstage[i]) (void)hipFree(h->d_mstage[i]);
        if (h->stage_free[i]) (void)hipEventDestroy(h->stage_free[i]);
    }
    if (h->d_counts) (void)hipFree(h->d_counts);  // (d_neg and d_maxmass live in the same block)
    if (h->own) (void)hipStreamDestroy(h->own);
    delete h;
    return SLICER_OK;
}

int slicer_set_option(slicer_handle h, const char *key, int32_t value)
{
    if (!h || !key)
        return fail(h, SLICER_ERR_ARG, "null argument");
    // (a pass stays "open" until the next slicer_plane_begin so that its maps can be read; what must not see a knob
    // change is work in flight: an open file, or binned chunks still waiting for their tile launch)
    bool busy = h->in_file;
    for (auto &Q : h->pg)
        busy = busy || Q.L.n > 0;
    if (busy)
        return fail(h, SLICER_ERR_STATE, "slicer_set_option with deposits in flight (open file or pending chunks)");
    for (const OptionName &o : kOptionNames)
        if (!strcmp(o.key, key)) {
            h->opt.*(o.field) = value;
            return SLICER_OK;
        }
    return fail(h, SLICER_ERR_ARG, "unknown option '%s'", key);
}

int slicer_get_option(slicer_handle h, const char *key, int32_t *value)
{
    if (!h || !key || !value)
        return fail(h, SLICER_ERR_ARG, "null argument");
    for (const OptionName &o : kOptionNames)
        if (!strcmp(o.key, key)) {
            *value = h->opt.*(o.field);
            return SLICER_OK;
        }
    return fail(h, SLICER_ERR_ARG, "unknown option '%s'", key);
}

int slicer_set_stream(slicer_handle h, void *hip_stream)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    // (a pass stays "open" after slicer_plane_finalize so that its maps can be read: what must not see the stream change
    // is a pass that still takes deposits)
    if (h->in_plane && !h->finalized)
        return fail(h, SLICER_ERR_STATE,
                    "cannot change stream inside a plane pass (between slicer_plane_begin and slicer_plane_finalize)");
    hipStream_t to = hip_stream ? (hipStream_t)hip_stream : h->own;
    if (to == h->stream)
        return SLICER_OK;
    // Everything this handle and its sub-handles queued on the old stream (finalize kernels, table uploads of a
    // *_create, runs) comes before whatever they queue on the new one: one event, recorded there and waited for here.
    HIPCHK(h, hipSetDevice(h->device));
    hipEvent_t e = get_event(h);
    if (!e)
        return fail(h, SLICER_ERR_HIP, "slicer_set_stream: no event to order the new stream behind the old one");
    hipError_t rc = hipEventRecord(e, h->stream);
    if (rc == hipSuccess)
        rc = hipStreamWaitEvent(to, e, 0);
    h->ev_pool.push_back(e);  // (the wait holds what the event stood for when it was queued: the event is free again)
    if (rc != hipSuccess)
        return fail(h, SLICER_ERR_HIP, "slicer_set_stream: ordering the streams failed: %s", hipGetErrorString(rc));
    h->stream = to;
    return SLICER_OK;
}

int slicer_plane_begin(slicer_handle h, const slicer_plane_desc *desc)
{
    if (!h || !desc)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (desc->npix <= 0 || desc->npix > 65536)
        return fail(h, SLICER_ERR_ARG, "npix %d out of range", desc->npix);
    if (desc->n_planes < 1 || desc->n_planes > SLICER_MAX_PLANES)
        return fail(h, SLICER_ERR_ARG, "n_planes %d out of range 1..%d", desc->n_planes, SLICER_MAX_PLANES);
    if (desc->mas != SLICER_MAS_TSC && desc->mas != SLICER_MAS_NGP)
        return fail(h, SLICER_ERR_ARG, "unknown mass-assignment scheme %d", desc->mas);
    if (desc->accum < SLICER_ACC_F32 || desc->accum > SLICER_ACC_FIXED64)
        return fail(h, SLICER_ERR_ARG, "unknown accumulator %d", desc->accum);
    if (desc->snopt < 0 || desc->snopt > 30)
        return fail(h, SLICER_ERR_ARG, "snopt = %d out of range 0..30", desc->snopt);
    if (!(desc->fov_rad > 0))
        return fail(h, SLICER_ERR_ARG, "fov_rad must be > 0");
    for (int p = 0; p < desc->n_planes; p++)
        if (desc->nrepperp[p] < 0 || desc->nrepperp[p] > 8)
            return fail(h, SLICER_ERR_ARG, "nrepperp[%d] = %d out of range 0..8", p, desc->nrepperp[p]);
    // shot-noise thinning in process-global mode: libc's stream is read here, before this call touches the HIP runtime
    pass_stream_return(h);  // (a pass that was never read or flushed)
    if (desc->snopt > 0 && !h->rand_private && libc_rand_grab(h->rand_state))
        h->rand_pass = true;
    HIPCHK(h, hipSetDevice(h->device));
    h->desc = *desc;
    h->dl_quot_ok = false;
    if (!is_pow2(desc->npix) && h->opt.dl_quot) {
        int rcq = dl_quotient_ok(h, desc->npix, h->dl_quot_ok);
        if (rcq)
            return rcq;
    }
    h->npix2 = (uint64_t)desc->npix * (uint64_t)desc->npix;
    h->in_plane = true;
    h->in_file = false;
    h->finalized = false;
    h->shared_seen = false;
    h->fixed_shared_set = false;
    h->algo_mask = 0;
    thin_drop(h);
    h->neg_remote = false;
    for (auto &Q : h->pg) {
        Q.L.n = 0;
        Q.key = -1;
        Q.particles = 0;
    }
    for (int t = 0; t < 6; t++) {
        h->type_seen[t] = false;
        h->fixed_exp_set[t] = false;
        h->file_mode[t] = 0;
    }
    zero_begin(h);
    int rcp = SLICER_OK;
    for (int p = 0; p < desc->n_planes && !rcp; p++) {
        rcp = ensure(h, h->planes[p].tot, h->npix2 * 4);
        if (!rcp && desc->mas == SLICER_MAS_NGP)  // the NGP fold accumulates into tot; TSC finalize overwrites it
            rcp = zero_async(h, h->planes[p].tot.p, h->npix2 * 4);
    }
    const int rcz = zero_end(h);
    if (rcp || rcz)
        return rcp ? rcp : rcz;
    HIPCHK(h, hipMemsetAsync(h->d_counts, 0, kPassScalarsBytes, h->stream));  // counters, guard flag, mass maxima
    return SLICER_OK;
}

int slicer_file_begin(slicer_handle h, const slicer_file_desc *file)
{
    if (!h || !file)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (!h->in_plane || h->finalized)
        return fail(h, SLICER_ERR_STATE, "slicer_file_begin outside a plane pass");
    if (h->in_file)
        return fail(h, SLICER_ERR_STATE, "slicer_file_begin: previous file not ended");
    if (!(file->boxsize > 0))
        return fail(h, SLICER_ERR_ARG, "boxsize must be > 0");
    for (int a = 0; a < 3; a++)
        if (file->sgn[a] != 1 && file->sgn[a] != -1)
            return fail(h, SLICER_ERR_ARG, "sgn[%d] = %d is not +-1", a, file->sgn[a]);
    // A constant header mass that is NaN, negative or infinite belongs to a corrupt header and would poison every pixel
    // the species touches; refused here, so that no constant-mass kernel has to test for it.  (0 is the hydro types'
    // "masses follow per particle"; a finite value above MAX_M is deposited as is, as in the reference.)
    for (int t = 0; t < 6; t++)
        if (file->npart[t] > 0 && !(file->massarr[t] >= 0.0 && file->massarr[t] <= DBL_MAX))
            return fail(h, SLICER_ERR_ARG, "slicer_file_begin: massarr[%d] = %g is negative or not finite", t,
                        file->massarr[t]);
    h->file = *file;
    h->in_file = true;
    h->file_serial++;
    for (int t = 0; t < 6; t++) {
        h->file_mode[t] = 0;
        h->file_partial_flush[t] = false;
    }
    return SLICER_OK;
}

int slicer_deposit_device(slicer_handle h, int type, const float *d_pos, const float *d_mass, uint64_t n)
{
    int rc = check_deposit_args(h, type, d_pos, d_mass, n);
    if (rc)
        return rc;
    if (n == 0)
        return SLICER_OK;
    HIPCHK(h, hipSetDevice(h->device));
    rc = begin_type(h, type, d_mass != nullptr);
    if (rc)
        return rc;
    // one kernel pass per max_chunk particles keeps the workspace bounded
    for (uint64_t off = 0; off < n; off += h->max_chunk) {
        uint64_t c = std::min<uint64_t>(h->max_chunk, n - off);
        rc = deposit_device_chunk(h, type, d_pos + 3 * off, d_mass ? d_mass + off : nullptr, c);
        if (rc)
            return rc;
    }
    return SLICER_OK;
}

namespace {
struct HostSpan {
    const float *pos;
    const float *mass;
};
int copy_fill(void *user, float *dst_pos, float *dst_mass, uint64_t first, uint64_t count)
{
    const HostSpan *s = static_cast<const HostSpan *>(user);
    memcpy(dst_pos, s->pos + 3 * first, count * 12);
    if (dst_mass)
        memcpy(dst_mass, s->mass + first, count * 4);
    return 0;
}
}  // namespace

int slicer_deposit_stream(slicer_handle h, int type, uint64_t n, int has_mass, slicer_fill_fn fill, void *user)
{
    int rc = check_deposit_args(h, type, fill ? (const void *)h : nullptr, nullptr, n);
    if (rc)
        return rc;
    if (n == 0)
        return SLICER_OK;
    if (!fill)
        return fail(h, SLICER_ERR_ARG, "null fill callback");
    HIPCHK(h, hipSetDevice(h->device));
    rc = begin_type(h, type, has_mass != 0);
    if (rc)
        return rc;
    rc = ensure_staging(h, has_mass != 0);
    if (rc)
        return rc;
    int slot = 0;
    for (uint64_t off = 0; off < n; off += h->stage_cap, slot ^= 1) {
        uint64_t c = std::min<uint64_t>(h->stage_cap, n - off);
        // the slot is reusable once the kernel that read it has finished; meanwhile the other slot's
        // H2D copy and kernels run, so filling (file read) overlaps with device work
        HIPCHK(h, hipEventSynchronize(h->stage_free[slot]));
        if (fill(user, h->h_stage[slot], has_mass ? h->h_mstage[slot] : nullptr, off, c) != 0)
            return fail(h, SLICER_ERR_ARG, "fill callback failed at particle %llu", (unsigned long long)off);
        HIPCHK(h, hipMemcpyAsync(h->d_stage[slot], h->h_stage[slot], c * 12, hipMemcpyHostToDevice, h->stream));
        const float *dm = nullptr;
        if (has_mass) {
            HIPCHK(h, hipMemcpyAsync(h->d_mstage[slot], h->h_mstage[slot], c * 4, hipMemcpyHostToDevice, h->stream));
            dm = h->d_mstage[slot];
        }
        rc = deposit_device_chunk(h, type, h->d_stage[slot], dm, c);
        if (rc)
            return rc;
        HIPCHK(h, hipEventRecord(h->stage_free[slot], h->stream));
    }
    return SLICER_OK;
}

int slicer_deposit_host(slicer_handle h, int type, const float *pos, const float *mass, uint64_t n)
{
    int rc = check_deposit_args(h, type, pos, mass, n);
    if (rc)
        return rc;
    HostSpan span{pos, mass};
    return slicer_deposit_stream(h, type, n, mass != nullptr, copy_fill, &span);
}

int slicer_file_end(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_file)
        return fail(h, SLICER_ERR_STATE, "slicer_file_end without slicer_file_begin");
    h->in_file = false;
    if (thin_deferred(h)) {  // deposited (and folded) plane by plane in thin_replay
        slicer_handle_s::ThinFile f;
        f.file = h->file;
        for (int t = 0; t < 6; t++) {
            f.mode[t] = h->file_mode[t];
            f.mconst[t] = h->file_mconst[t];
        }
        h->thin_files.push_back(f);
        return SLICER_OK;
    }
    if (h->desc.mas == SLICER_MAS_NGP) {
        for (auto &Q : h->pg)
            for (int c = 0; c < Q.L.n; c++)
                Q.L.done[c] = 1;  // every chunk still pending belongs to a closed file now
        // A species whose counts all wait in the pending lists marked `fold` needs nothing more here: the tile kernel
        // folds them, file by file, when the lists are flushed (NgpFold).  Anything else has counts in the global count
        // maps (or is about to: its pending chunks carry fold = 0) and is folded by the map-wide kernel, now.
        bool need_kernel = false;
        for (int t = 0; t < 6; t++) {
            if (!h->file_mode[t])
                continue;
            if (h->file_mode[t] == 1 && ngp_foldable(h, t))
                h->file_mode[t] = 0;
            else
                need_kernel = true;
        }
        if (need_kernel) {
            int rcf = flush_pending(h);
            if (rcf)
                return rcf;
            for (int p = 0; p < h->desc.n_planes; p++) {
                int rc = fold_file_plane(h, p);
                if (rc)
                    return rc;
            }
        }
    }
    return SLICER_OK;
}

int slicer_plane_finalize(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_finalize outside a plane pass");
    if (h->in_file)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_finalize: file not ended");
    if (h->finalized)
        return SLICER_OK;
    const slicer_plane_desc &d = h->desc;
    {
        int rcf = thin_replay(h);
        if (!rcf)
            rcf = flush_pending(h);
        if (rcf)
            return rcf;
    }
    if (d.mas == SLICER_MAS_TSC) {
        const int kind = acc_kind(d, false);
        for (int p = 0; p < d.n_planes; p++) {
            FinalizeArgs A;
            memset(&A, 0, sizeof A);
            bool any = false;
            if (!d.want_type_maps && kind == kF32 && h->shared_seen) {
                // the shared f32 accumulator already is the all-types map: hand the buffer over instead of copying
                std::swap(h->planes[p].tot, h->planes[p].acc_shared);
                continue;
            }
            if (!d.want_type_maps) {
                A.acc_shared = h->shared_seen ? h->planes[p].acc_shared.p : nullptr;
                A.inv_scale_shared = std::ldexp(1.0, -h->fixed_exp_shared);
                any = h->shared_seen;
            } else {
                for (int t = 0; t < 6; t++) {
                    if (!h->type_seen[t])
                        continue;
                    any = true;
                    A.acc[t] = kind == kF32 ? h->planes[p].toti[t].p : h->planes[p].acc[t].p;
                    A.toti[t] = (float *)h->planes[p].toti[t].p;
                    A.inv_scale[t] = std::ldexp(1.0, -h->fixed_exp[t]);
                }
            }
            A.tot = (float *)h->planes[p].tot.p;
            A.npix2 = h->npix2;
            if (!any) {
                int rc = zero_async(h, A.tot, h->npix2 * 4);
                if (rc)
                    return rc;
                continue;
            }
            ProfScope ps(h, KN_FINALIZE);
            HIPCHK(h, launch_finalize_tsc(kind, A, h->stream));
        }
    }
    h->finalized = true;
    return SLICER_OK;
}

int slicer_plane_device_maps(slicer_handle h, int plane, float **d_tot, float **d_toti)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane || !h->finalized)
        return fail(h, SLICER_ERR_STATE, "maps are available after slicer_plane_finalize");
    if (plane < 0 || plane >= h->desc.n_planes)
        return fail(h, SLICER_ERR_ARG, "plane %d out of range", plane);
    if (d_tot)
        *d_tot = (float *)h->planes[plane].tot.p;
    if (d_toti)
        for (int t = 0; t < 6; t++)
            d_toti[t] = (h->type_seen[t] && h->desc.want_type_maps) ? (float *)h->planes[plane].toti[t].p : nullptr;
    return SLICER_OK;
}

int slicer_get_stream(slicer_handle h, void **hip_stream)
{
    if (!h || !hip_stream)
        return fail(h, SLICER_ERR_ARG, "null argument");
    *hip_stream = (void *)h->stream;
    return SLICER_OK;
}

int slicer_plane_info(slicer_handle h, int32_t *npix, int32_t *n_planes)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane)
        return fail(h, SLICER_ERR_STATE, "no plane pass is open");
    if (npix)
        *npix = h->desc.npix;
    if (n_planes)
        *n_planes = h->desc.n_planes;
    return SLICER_OK;
}

int slicer_plane_device_counts(slicer_handle h, int plane, uint64_t **d_counts)
{
    if (!h || !d_counts)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (plane < 0 || plane >= SLICER_MAX_PLANES)
        return fail(h, SLICER_ERR_ARG, "plane %d out of range", plane);
    *d_counts = (uint64_t *)(h->d_counts + (size_t)plane * 6);
    return SLICER_OK;
}

int slicer_plane_algo_mask(slicer_handle h, int32_t *mask)
{
    if (!h || !mask)
        return fail(h, SLICER_ERR_ARG, "null argument");
    *mask = h->algo_mask;
    return SLICER_OK;
}

int slicer_plane_status(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_status outside a plane pass");
    HIPCHK(h, hipSetDevice(h->device));
    int neg = 0;
    HIPCHK(h, hipMemcpyAsync(&neg, h->d_neg, sizeof neg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (neg || h->neg_remote)
        return fail(h, SLICER_ERR_NEGATIVE_COORD,
                    "a transformed coordinate is negative (positions outside [0, 2*boxsize]?): the reference stops "
                    "here (densitymaps.cpp:334-345)%s", neg ? "" : " [reported by another rank]");
    return SLICER_OK;
}

int slicer_plane_flush(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane || h->in_file)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_flush: needs an open plane pass and no open file");
    if (h->finalized)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_flush after slicer_plane_finalize");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = thin_replay(h);
    return rc ? rc : flush_pending(h);
}

int slicer_synchronize(slicer_handle h)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SLICER_OK;
}

int slicer_plane_read(slicer_handle h, int plane, float *tot, float *toti, int64_t *nsel)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (!h->in_plane)
        return fail(h, SLICER_ERR_STATE, "slicer_plane_read outside a plane pass");
    if (plane < 0 || plane >= h->desc.n_planes)
        return fail(h, SLICER_ERR_ARG, "plane %d out of range", plane);
    int rc = slicer_plane_finalize(h);
    if (rc)
        return rc;
    rc = slicer_plane_status(h);  // synchronises; densitymaps.cpp:334-345
    if (rc)
        return rc;
    const size_t n4 = h->npix2 * 4;
    if (tot && (rc = copy_map_to_host(h, tot, h->planes[plane].tot.p, n4)))
        return rc;
    if (toti) {
        for (int t = 0; t < 6; t++) {
            if (h->type_seen[t] && h->desc.want_type_maps) {
                if ((rc = copy_map_to_host(h, toti + h->npix2 * t, h->planes[plane].toti[t].p, n4)))
                    return rc;
            } else {
                memset(toti + h->npix2 * t, 0, n4);
            }
        }
    }
    if (nsel) {
        unsigned long long c[6];
        HIPCHK(h, hipMemcpy(c, h->d_counts + (size_t)plane * 6, sizeof c, hipMemcpyDeviceToHost));
        for (int t = 0; t < 6; t++)
            nsel[t] = (int64_t)c[t];
    }
    return SLICER_OK;
}

int slicer_device_malloc(slicer_handle h, size_t bytes, void **d_ptr)
{
    if (!h || !d_ptr)
        return fail(h, SLICER_ERR_ARG, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMalloc(d_ptr, bytes));
    return SLICER_OK;
}

int slicer_device_free(slicer_handle h, void *d_ptr)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipFree(d_ptr));
    return SLICER_OK;
}

int slicer_copy_to_device(slicer_handle h, void *d_dst, const void *src, size_t bytes)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    HIPCHK(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SLICER_OK;
}

int slicer_copy_to_host(slicer_handle h, void *dst, const void *d_src, size_t bytes)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return copy_map_to_host(h, dst, d_src, bytes);
}

int slicer_synth_positions(slicer_handle h, float *d_pos, uint64_t first, uint64_t count, double boxsize,
                           uint64_t seed, int clustered)
{
    if (!h || (!d_pos && count))
        return fail(h, SLICER_ERR_ARG, "null argument");
    ProfScope ps(h, KN_SYNTH);
    HIPCHK(h, launch_synth(d_pos, first, count, boxsize, seed, clustered, h->stream));
    return SLICER_OK;
}

}  // extern "C"
