// reduce_meta.cpp -- what ranks that own different sub-files of a pass exchange before their accumulators are summed:
// which accumulators are live, their FIXED64 scales, the negativity guard.
#include "slicer_host.hpp"

#include <cstdint>

namespace {

// which accumulator slots (types 0..5, 6 = shared / all-types) take part in a cross-rank sum, and their element kind
void reduce_slots(slicer_handle h, bool live[7], int &elem)
{
    const slicer_plane_desc &d = h->desc;
    for (int s = 0; s < 7; s++)
        live[s] = false;
    if (d.mas == SLICER_MAS_NGP) {
        // the per-file fold (densitymaps.cpp:511-513) already produced f32 maps: they are what the reference sums
        elem = SLICER_ELEM_F32;
        live[6] = true;
        if (d.want_type_maps)
            for (int t = 0; t < 6; t++)
                live[t] = h->type_seen[t];
        return;
    }
    elem = d.accum == SLICER_ACC_F64 ? SLICER_ELEM_F64 : d.accum == SLICER_ACC_FIXED64 ? SLICER_ELEM_FIXED64 : SLICER_ELEM_F32;
    if (!d.want_type_maps) {
        live[6] = h->shared_seen;
        return;
    }
    for (int t = 0; t < 6; t++)
        live[t] = h->type_seen[t];
}

// the host-known part of the reduce meta: which accumulators are live and their FIXED64 scales (v[21..23] = 0)
int reduce_meta_local(slicer_handle h, slicer_reduce_meta *m, const char *who)
{
    if (!h || !m)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (!h->in_plane || h->in_file || h->finalized)
        return fail(h, SLICER_ERR_STATE, "%s: after the last slicer_file_end, before finalize", who);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = thin_replay(h);
    if (!rc)
        rc = flush_pending(h);
    if (rc)
        return rc;
    bool live[7];
    int elem;
    reduce_slots(h, live, elem);
    for (int s = 0; s < 7; s++) {
        m->v[s] = live[s] ? 1 : 0;
        const bool fx = live[s] && elem == SLICER_ELEM_FIXED64;
        const int e = s < 6 ? h->fixed_exp[s] : h->fixed_exp_shared;
        m->v[7 + s] = fx ? e : INT32_MIN;
        m->v[14 + s] = fx ? -e : INT32_MIN;
    }
    m->v[21] = m->v[22] = m->v[23] = 0;
    return SLICER_OK;
}

}  // namespace

extern "C" {

int slicer_reduce_meta_get(slicer_handle h, slicer_reduce_meta *m)
{
    int rc = reduce_meta_local(h, m, "slicer_reduce_meta_get");
    if (rc)
        return rc;
    int neg = 0;
    HIPCHK(h, hipMemcpyAsync(&neg, h->d_neg, sizeof neg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    m->v[21] = neg ? 1 : 0;
    return SLICER_OK;
}

int slicer_reduce_meta_get_async(slicer_handle h, slicer_reduce_meta *m)
{
    return reduce_meta_local(h, m, "slicer_reduce_meta_get_async");
}

int slicer_plane_device_guard(slicer_handle h, int32_t **d_flag)
{
    if (!h || !d_flag)
        return fail(h, SLICER_ERR_ARG, "null argument");
    *d_flag = (int32_t *)h->d_neg;
    return SLICER_OK;
}

int slicer_reduce_meta_set(slicer_handle h, const slicer_reduce_meta *m)
{
    if (!h || !m)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (!h->in_plane || h->in_file || h->finalized)
        return fail(h, SLICER_ERR_STATE, "slicer_reduce_meta_set: after the last slicer_file_end, before finalize");
    HIPCHK(h, hipSetDevice(h->device));
    const slicer_plane_desc &d = h->desc;
    bool live[7];
    int elem;
    reduce_slots(h, live, elem);
    const bool ngp = d.mas == SLICER_MAS_NGP;
    const size_t esz = elem == SLICER_ELEM_F32 ? 4 : 8;
    for (int s = 0; s < 7; s++) {
        if (!m->v[s])
            continue;
        if (elem == SLICER_ELEM_FIXED64) {
            if (m->v[7 + s] == INT32_MIN || m->v[7 + s] != -m->v[14 + s])
                return fail(h, SLICER_ERR_UNSUPPORTED,
                            "ranks scaled FIXED64 accumulator %d differently (2^%d vs 2^%d): their integer sums cannot be "
                            "added; pass the same mass table on every rank", s, m->v[7 + s], -m->v[14 + s]);
            if (live[s] && (s < 6 ? h->fixed_exp[s] : h->fixed_exp_shared) != m->v[7 + s])
                return fail(h, SLICER_ERR_UNSUPPORTED, "FIXED64 scale of accumulator %d differs from the combined one", s);
        }
        if (live[s])
            continue;
        // this rank never saw the slot: zero-filled stand-ins keep the set of collectives rank-invariant
        const bool shared_layout = !ngp && !d.want_type_maps;
        const bool valid = s == 6 ? shared_layout : (ngp ? d.want_type_maps != 0 : !shared_layout);
        if (!valid)
            return fail(h, SLICER_ERR_ARG, "combined reduce meta names accumulator %d, which this pass layout lacks", s);
        for (int p = 0; p < d.n_planes; p++) {
            int rc;
            if (s == 6) {  // shared TSC accumulator (NGP's slot 6 is tot: always live)
                if ((rc = ensure(h, h->planes[p].acc_shared, h->npix2 * esz)) ||
                    (rc = zero_async(h, h->planes[p].acc_shared.p, h->npix2 * esz)))
                    return rc;
            } else {
                if ((rc = ensure(h, h->planes[p].toti[s], h->npix2 * 4)) ||
                    (rc = zero_async(h, h->planes[p].toti[s].p, h->npix2 * 4)))
                    return rc;
                if (!ngp && elem != SLICER_ELEM_F32 &&
                    ((rc = ensure(h, h->planes[p].acc[s], h->npix2 * esz)) ||
                     (rc = zero_async(h, h->planes[p].acc[s].p, h->npix2 * esz))))
                    return rc;
            }
        }
        if (s == 6) {
            h->shared_seen = true;
            h->fixed_exp_shared = elem == SLICER_ELEM_FIXED64 ? m->v[7 + s] : h->fixed_exp_shared;
            h->fixed_shared_set = true;
        } else {
            h->type_seen[s] = true;
            if (elem == SLICER_ELEM_FIXED64)
                h->fixed_exp[s] = m->v[7 + s];
            h->fixed_exp_set[s] = true;
        }
    }
    h->neg_remote = m->v[21] != 0;
    return SLICER_OK;
}

int slicer_plane_accumulators(slicer_handle h, int plane, void **acc, int32_t *elem_kind)
{
    if (!h || !acc || !elem_kind)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (!h->in_plane || h->in_file || h->finalized)
        return fail(h, SLICER_ERR_STATE, "accumulators are available after the last slicer_file_end, before finalize");
    if (plane < 0 || plane >= h->desc.n_planes)
        return fail(h, SLICER_ERR_ARG, "plane %d out of range", plane);
    for (auto &Q : h->pg)
        if (Q.L.n)
            return fail(h, SLICER_ERR_STATE, "call slicer_plane_flush (or slicer_reduce_meta_get) first");
    bool live[7];
    int elem;
    reduce_slots(h, live, elem);
    const bool ngp = h->desc.mas == SLICER_MAS_NGP;
    for (int s = 0; s < 7; s++) {
        acc[s] = nullptr;
        if (!live[s])
            continue;
        if (s == 6)
            acc[s] = ngp ? h->planes[plane].tot.p : h->planes[plane].acc_shared.p;
        else
            acc[s] = (ngp || elem == SLICER_ELEM_F32) ? h->planes[plane].toti[s].p : h->planes[plane].acc[s].p;
    }
    *elem_kind = elem;
    return SLICER_OK;
}

}  // extern "C"
