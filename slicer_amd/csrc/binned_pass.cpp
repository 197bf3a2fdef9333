// binned_pass.cpp -- one chunk of particles through the device: the clearing of a pass's maps, the workspaces and the
// pending lists of the binned pipeline (project+bin, sort, one tile launch per list), the choice between it and the
// fused global-atomic kernel, and the NGP per-file fold.
#include "slicer_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace slicer;

namespace {

size_t acc_elem_size(int kind) { return (kind == kF64 || kind == kFixed64) ? 8 : 4; }

// Zero-fills on the handle's stream.  Between zero_begin and zero_end they are collected and go out as ONE launch
// (launch_zero_many): a pass clears four to fourteen maps, and every dispatch costs a few microseconds of idle GPU.
int zero_flush(slicer_handle h)
{
    ZeroList &Z = h->zero_list;
    if (Z.n == 1) {
        HIPCHK(h, hipMemsetAsync(Z.p[0], 0, Z.words[0] * 4, h->stream));
    } else if (Z.n > 1) {
        HIPCHK(h, launch_zero_many(Z, h->stream));
    }
    Z.n = 0;
    Z.quad0[0] = 0;
    return SLICER_OK;
}


}  // namespace

int zero_async(slicer_handle h, void *p, size_t bytes)
{
    if (!h->zero_collect || (bytes & 3) || bytes == 0) {
        HIPCHK(h, hipMemsetAsync(p, 0, bytes, h->stream));
        return SLICER_OK;
    }
    ZeroList &Z = h->zero_list;
    if (Z.n == kZeroMax) {
        int rc = zero_flush(h);
        if (rc)
            return rc;
    }
    Z.p[Z.n] = p;
    Z.words[Z.n] = bytes / 4;
    Z.quad0[Z.n + 1] = Z.quad0[Z.n] + (bytes / 4 + 3) / 4;
    Z.n++;
    return SLICER_OK;
}

void zero_begin(slicer_handle h)
{
    h->zero_collect = h->opt.zero_batch != 0;
    h->zero_list.n = 0;
    h->zero_list.quad0[0] = 0;
}

int zero_end(slicer_handle h)
{
    h->zero_collect = false;
    return zero_flush(h);
}

namespace {

// Make sure the destination buffers of `type` exist and are zeroed for this plane pass.
int prepare_type_maps(slicer_handle h, int type, bool has_mass)
{
    const slicer_plane_desc &d = h->desc;
    const size_t n4 = h->npix2 * 4;
    const int kind = acc_kind(d, has_mass);
    const bool ngp = d.mas == SLICER_MAS_NGP;
    const bool shared = !ngp && !d.want_type_maps;
    if (shared) {
        if (!h->shared_seen) {
            if (!h->fixed_shared_set) {
                // From the mass table alone, which every sub-file of a snapshot carries identically -- not from which
                // types this particular file holds -- so that ranks owning different sub-files pick the same scale
                // (their FIXED64 accumulators are summed as integers: slicer_plane_accumulators).
                double mm = 0;
                for (int t = 0; t < 6; t++)
                    mm = std::max(mm, h->file.massarr[t]);
                h->fixed_exp_shared = pick_fixed_exp(d, mm, d.hydro != 0);
                h->fixed_shared_set = true;
            }
            for (int p = 0; p < d.n_planes; p++) {
                int rc = ensure(h, h->planes[p].acc_shared, h->npix2 * acc_elem_size(kind));
                if (rc)
                    return rc;
                rc = zero_async(h, h->planes[p].acc_shared.p, h->npix2 * acc_elem_size(kind));
                if (rc)
                    return rc;
            }
            h->shared_seen = true;
        }
        return SLICER_OK;
    }
    if (!h->type_seen[type]) {
        if (!h->fixed_exp_set[type]) {
            h->fixed_exp[type] = pick_fixed_exp(d, h->file.massarr[type], has_mass);
            h->fixed_exp_set[type] = true;
        }
        for (int p = 0; p < d.n_planes; p++) {
            int rc = SLICER_OK;
            if (!ngp || d.want_type_maps) {  // NGP without per-type outputs only needs the count scratch
                rc = ensure(h, h->planes[p].toti[type], n4);
                if (rc)
                    return rc;
                rc = zero_async(h, h->planes[p].toti[type].p, n4);
                if (rc)
                    return rc;
            }
            if (ngp || kind != kF32) {
                size_t b = h->npix2 * (ngp ? 4 : acc_elem_size(kind));
                rc = ensure(h, h->planes[p].acc[type], b);
                if (rc)
                    return rc;
                rc = zero_async(h, h->planes[p].acc[type].p, b);
                if (rc)
                    return rc;
            }
        }
        h->type_seen[type] = true;
    }
    return SLICER_OK;
}


// persistent K3 workgroups: two per CU (their LDS and registers allow it), so that one workgroup's load / LDS /
// store phases overlap the other's; option k3_per_cu overrides (tuning knob)
int scatter_workgroups(slicer_handle h)
{
    return h->num_cus * std::max(1, h->opt.k3_per_cu);
}

int ensure_bin_workspace(slicer_handle h, bool has_mass, int group, int slot, uint64_t n, const BinGeom &G,
                         BinWorkspace &W)
{
    auto &Q = h->pg[group];
    const uint64_t nb = (n + G.batch - 1) / G.batch;
    const uint64_t region = (uint64_t)G.n_units * nb * G.region;  // compact records: [unit][workgroup][region]
    const uint64_t nrec = n * (uint64_t)(G.region / G.batch);     // most records this chunk can emit
    int rc;
    if ((rc = ensure(h, h->w_cxy, region * 8)) || (rc = ensure(h, h->w_cbin, region * 2)) ||
        (rc = ensure(h, h->w_hist, nb * (uint64_t)G.nbins * 4)) ||
        (rc = ensure(h, h->w_hist16, nb * (uint64_t)(G.nbins + 2) * 2)) ||
        (rc = ensure(h, h->w_total, (kMaxBins + kMaxBins / 32 + 1) * 4)) ||
        (rc = ensure(h, h->w_bcount, nb * kMaxUnits * 4)) || (rc = ensure(h, Q.w_sxy[slot], nrec * (has_mass ? 12 : 8))) ||  // float2, or Rec3 with per-particle masses
        (rc = ensure(h, Q.w_base[slot], (kMaxBins + 1) * 4)))
        return rc;
    if (has_mass && (rc = ensure(h, h->w_cm, region * 4)))
        return rc;
    W.cxy = (float2 *)h->w_cxy.p;
    W.cbin = (unsigned short *)h->w_cbin.p;
    W.cm = (float *)h->w_cm.p;
    W.sxy = (float2 *)Q.w_sxy[slot].p;
    W.sm = has_mass ? (float *)Q.w_sxy[slot].p : nullptr;  // (the masses travel inside the 12-byte sorted records)
    W.hist = (unsigned *)h->w_hist.p;
    W.hist16 = (unsigned *)h->w_hist16.p;
    W.total = (unsigned *)h->w_total.p;
    W.base = (unsigned *)Q.w_base[slot].p;
    W.bcount = (unsigned *)h->w_bcount.p;
    return SLICER_OK;
}

// Two-level sort: the units of the pass become coarse bins -- bands of 2^crow_log2 tile rows of one plane -- chosen so
// that a pass has about 64 of them (runs of ~0.5 KB in the project+bin kernel's sub-batches as well as in the sort
// kernel's items) within the 8-bit ids of both kernels.  False if the pass does not fit (the one-level sort serves it).
bool sort2_geom(const BinGeom &G, int n_planes, BinGeom &G2, int &crow_log2)
{
    G2 = G;
    crow_log2 = 0;
    auto units = [&](int cl) { return n_planes * ((G.nty + (1 << cl) - 1) >> cl); };
    while (units(crow_log2) > 64 && (2 << crow_log2) * G.ntx <= kMaxCoarseTiles)
        crow_log2++;
    G2.rows_per_unit = 1 << crow_log2;
    G2.units_per_plane = (G.nty + G2.rows_per_unit - 1) / G2.rows_per_unit;
    G2.tiles_per_unit = G2.rows_per_unit * G.ntx;
    G2.n_units = n_planes * G2.units_per_plane;
    G2.nbins = G2.n_units * G2.tiles_per_unit;
    return G2.n_units <= kMaxCoarse && G2.tiles_per_unit <= kMaxCoarseTiles && G.region == G.batch && G.batch <= 32768;
}

constexpr int kSort2Slots = kSort2Blocks * kSubBatches;  // sub-batch slots per item of the sort kernel

int ensure_sort2_workspace(slicer_handle h, int group, int slot, uint64_t n, const BinGeom &G, int ngroups, BinWorkspace &W)
{
    auto &Q = h->pg[group];
    const uint64_t nb = (n + G.batch - 1) / G.batch, nslots = nb * kSubBatches;
    int rc;
    bool fresh_tot = false;
    if ((rc = ensure(h, h->w_c1, nb * (uint64_t)G.batch * 8)) || (rc = ensure(h, h->w_sboff, nslots * 4)) ||
        (rc = ensure(h, h->w_sbstart, (uint64_t)kSubRow * nslots * 2)) || (rc = ensure(h, h->w_sbn, nb * 4)) ||
        (rc = ensure(h, Q.w_sxy[slot], n * 8)) || (rc = ensure(h, Q.w_base[slot], (kMaxBins + 1) * 4)) ||
        (rc = ensure(h, Q.w_ptab[slot], (uint64_t)G.n_units * ngroups * (G.tiles_per_unit + 1) * 4)) ||
        (rc = ensure(h, Q.w_tot, (uint64_t)kMaxCoarse * kMaxCoarseTiles * 4, &fresh_tot)))
        return rc;
    memset(&W, 0, sizeof W);
    W.c1 = (float2 *)h->w_c1.p;
    W.sb_off = (unsigned *)h->w_sboff.p;
    W.sb_start = (unsigned short *)h->w_sbstart.p;
    W.sb_n = (unsigned *)h->w_sbn.p;
    W.sxy = (float2 *)Q.w_sxy[slot].p;
    W.ptab = (unsigned *)Q.w_ptab[slot].p;
    W.item_tot = (unsigned *)Q.w_base[slot].p;
    W.tot = (unsigned *)Q.w_tot.p;
    W.base = (unsigned *)Q.w_base[slot].p;
    if (slot == 0 || fresh_tot)  // a new pending list starts from zero totals (the tile launch's item builder re-zeroes them)
        HIPCHK(h, hipMemsetAsync(W.tot, 0, (size_t)G.nbins * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(W.item_tot, 0, (size_t)ngroups * G.n_units * 4, h->stream));
    return SLICER_OK;
}

}  // namespace

int prepare_type(slicer_handle h, int type, bool has_mass)
{
    zero_begin(h);  // the maps of all planes are cleared by one launch
    const int rc = prepare_type_maps(h, type, has_mass);
    const int rcz = zero_end(h);
    return rc ? rc : rcz;
}

bool ngp_foldable(slicer_handle h, int type)
{
    int species = 0;
    for (int t = 0; t < 6; t++)
        species += h->file.npart[t] > 0;
    return species == 1 && h->file.npart[type] > 0 && !h->file_partial_flush[type] && !h->opt.ngp_general;
}

// NGP: some of the open file's records of this species are (about to be) in the global count map, so none of them may
// be folded inside the tile kernel: the per-file sum needs the file's complete count per pixel (k_fold_ngp does it)
void ngp_spoil_file(slicer_handle h, int type)
{
    h->file_partial_flush[type] = true;
    for (auto &Q : h->pg)
        if (Q.L.n && Q.key < 12 && Q.key / 2 == type)
            for (int c = 0; c < Q.L.n; c++)
                if (!Q.L.done[c])
                    Q.L.fold[c] = 0;
}

namespace {

// Deposit the pending (binned) chunks of one plane group with one tile-kernel launch.
int flush_group(slicer_handle h, int group)
{
    auto &Q = h->pg[group];
    if (Q.L.n == 0)
        return SLICER_OK;
    NgpFold F;
    memset(&F, 0, sizeof F);
    if (Q.cfg.mas == kNGP && Q.cfg.acc == kCountU32 && Q.key < 12) {
        const int ptype = Q.key / 2;
        for (int c = 0; c < Q.L.n; c++)
            if (!Q.L.done[c]) {  // a flush in mid-file: the open file's counts are partial
                ngp_spoil_file(h, ptype);
                break;
            }
        for (int c = 0; c < Q.L.n; c++)
            F.on |= Q.L.fold[c];
        for (int p = 0; p < Q.np; p++) {
            F.tot[p] = (float *)h->planes[Q.p0 + p].tot.p;
            F.toti[p] = h->desc.want_type_maps ? (float *)h->planes[Q.p0 + p].toti[ptype].p : nullptr;
        }
    }
    bool fresh = false;
    int rc = ensure(h, h->w_items, tile_items_bytes(Q.G, Q.particles), &fresh);
    if (rc)
        return rc;
    if (fresh) {  // fresh workspace: both work-item counters start at zero
        HIPCHK(h, hipMemsetAsync(h->w_items.p, 0, 16, h->stream));
        h->items_epoch = 0;
    }
    Q.L.run0[0] = 0;
    for (int c = 0; c < Q.L.n; c++)
        Q.L.run0[c + 1] = Q.L.run0[c] + (Q.L.ptab[c] ? Q.L.ngroups[c] : 1);
    Q.L.tot = Q.sort2 ? (unsigned *)Q.w_tot.p : nullptr;
    {
        ProfScope ps(h, KN_TILE);
        bool int_cells = false;
        HIPCHK(h, launch_tile_deposit(Q.cfg, Q.P, Q.G, Q.L, Q.T, F, h->w_items.p, h->items_epoch++, Q.particles,
                                      h->opt.k4_int, &int_cells, h->stream));
        if (int_cells)
            h->algo_mask |= 1 << 6;
    }
    Q.L.n = 0;
    Q.key = -1;
    Q.particles = 0;
    return SLICER_OK;
}

}  // namespace

int flush_pending(slicer_handle h)
{
    for (int g = 0; g < SLICER_MAX_PLANES; g++) {
        int rc = flush_group(h, g);
        if (rc)
            return rc;
    }
    return SLICER_OK;
}

// NGP: fold this file's per-type count / mass maps of plane p into its float maps (densitymaps.cpp:405-412 adds each
// file's mapxyi into the running maps)
int fold_file_plane(slicer_handle h, int p)
{
    bool any = false;
    for (int t = 0; t < 6; t++)
        any |= h->file_mode[t] != 0;
    if (!any)
        return SLICER_OK;
    FoldArgs A;
    memset(&A, 0, sizeof A);
    for (int t = 0; t < 6; t++) {
        A.mode[t] = h->file_mode[t];
        A.mconst[t] = h->file_mconst[t];
        A.scratch[t] = h->file_mode[t] ? h->planes[p].acc[t].p : nullptr;
        A.toti[t] = (h->file_mode[t] && h->desc.want_type_maps) ? (float *)h->planes[p].toti[t].p : nullptr;
    }
    A.tot = (float *)h->planes[p].tot.p;
    A.npix2 = h->npix2;
    ProfScope ps(h, KN_FOLD);
    HIPCHK(h, launch_fold_ngp(A, h->stream));
    return SLICER_OK;
}

namespace {

// One chunk through K1-K3 for the planes [p0, p0 + np) of the pass (P and T already hold them in slots 0 .. np - 1);
// the sorted records wait in the pending list for the tile kernel.
int binned_chunk(slicer_handle h, const LaunchCfg &cfg, const PassParams &P, const Targets &T, BinGeom G, int type,
                 int group, int p0, int np, const float *d_pos, const float *d_mass, uint64_t n)
{
    auto &Q = h->pg[group];
    const slicer_plane_desc &d = h->desc;
    const bool has_mass = d_mass != nullptr;
    if (!h->opt.bin_batch) {
        // K1 keeps two workgroups per CU resident: size the batch so that the workgroups of this call fill whole
        // rounds of resident slots instead of leaving a short tail round
        const uint64_t slots = 2ull * (uint64_t)h->num_cus;
        const uint64_t rounds = (n + slots * kBinBatch - 1) / (slots * kBinBatch);
        const uint64_t per = (n + slots * rounds - 1) / (slots * rounds);
        const int reps = G.region / G.batch;
        G.batch = (int)std::min<uint64_t>(G.batch, std::max<uint64_t>(std::min(8192, G.batch), (per + 1023) / 1024 * 1024));
        G.region = G.batch * reps;
    }
    const bool shared = d.mas != SLICER_MAS_NGP && !d.want_type_maps;
    const int key = (shared ? 12 : type * 2) + (has_mass ? 1 : 0);
    int rc;
    int nblocks = (int)((n + G.batch - 1) / G.batch);
    K1Args A;
    bool fast = false;
    if ((rc = k1_fast_args(h, P, G, nblocks, A, fast)))
        return rc;
    // two-level sort where the pass qualifies: the fast project+bin kernel without the wave stacks, constant mass, a unit
    // table within the 8-bit ids, at most kMaxSortGroups items per unit
    BinGeom G2;
    int crow_log2 = 0;
    const bool sort2 = fast && h->opt.sort2 && !has_mass && !A.stack && sort2_geom(G, P.n_planes, G2, crow_log2) &&
                       (nblocks * kSubBatches + kSort2Slots - 1) / kSort2Slots <= kMaxSortGroups;
    if (sort2) {
        G = G2;
        A.sort2 = 1;
        A.crow_log2 = crow_log2;
    }
    if (Q.L.n && (Q.key != key || Q.p0 != p0 || Q.np != np || Q.L.n >= Q.limit || Q.sort2 != sort2) &&
        (rc = flush_group(h, group)))
        return rc;
    const int slot = Q.L.n;
    BinWorkspace W;
    h->algo_mask |= fast ? (1 << 4) : (1 << 5);
    if (sort2) {
        const int ngroups = (nblocks * kSubBatches + kSort2Slots - 1) / kSort2Slots;
        if ((rc = ensure_sort2_workspace(h, group, slot, n, G, ngroups, W)))
            return rc;
        h->algo_mask |= 1 << 7;
        {
            ProfScope ps(h, KN_PROJECT);
            HIPCHK(h, launch_project_bin(cfg, true, d_pos, d_mass, n, P, A, G, W, T, h->stream));
        }
        {
            ProfScope ps(h, KN_SORT2);
            HIPCHK(h, launch_sort2(nblocks, kSort2Slots, ngroups, scatter_workgroups(h), P, G, W, h->stream));
        }
        Q.L.ptab[slot] = W.ptab;
        Q.L.ngroups[slot] = ngroups;
    } else {
        if ((rc = ensure_bin_workspace(h, has_mass, group, slot, n, G, W)))
            return rc;
        {
            ProfScope ps(h, KN_PROJECT);
            HIPCHK(h, launch_project_bin(cfg, fast, d_pos, d_mass, n, P, A, G, W, T, h->stream));
        }
        {
            ProfScope ps(h, KN_SCAN);
            HIPCHK(h, launch_bin_scan(cfg, nblocks, P.n_planes, G, W, T, h->stream));
        }
        {
            ProfScope ps(h, KN_SCATTER);
            HIPCHK(h, launch_bin_scatter(cfg, nblocks, P.n_planes, scatter_workgroups(h), G, W, T, h->stream));
        }
        Q.L.ptab[slot] = nullptr;
        Q.L.ngroups[slot] = 1;
    }
    if (slot == 0) {
        // chunks per tile launch: enough for ~16384 records per bin (what eight chunks of the headline case bring),
        // judged by the first chunk; option `pending` overrides
        const uint64_t per_bin = std::max<uint64_t>(1, n * (uint64_t)(G.region / G.batch) / (uint64_t)std::max(1, G.nbins));
        int limit = (int)std::min<uint64_t>(kMaxPending, std::max<uint64_t>(8, (16384 + per_bin - 1) / per_bin));
        if (h->opt.pending > 0)
            limit = std::min(h->opt.pending, kMaxPending);
        Q.limit = sort2 ? std::min(limit, kMaxPendingRuns) : limit;
        Q.key = key;
        Q.sort2 = sort2;
        Q.p0 = p0;
        Q.np = np;
        Q.cfg = cfg;
        Q.P = P;
        Q.G = G;
        Q.T = T;
    }
    Q.L.sxy[slot] = W.sxy;
    Q.L.sm[slot] = has_mass ? W.sm : nullptr;
    Q.L.base[slot] = W.base;
    Q.L.mconst[slot] = P.mconst;
    Q.L.file_id[slot] = (unsigned short)h->file_serial;
    Q.L.done[slot] = 0;
    Q.L.fold[slot] = cfg.mas == kNGP && cfg.acc == kCountU32 && ngp_foldable(h, type);
    if (Q.L.fold[slot] && G.tw_log2 + G.th_log2 > 14) {  // the tile kernel keeps 16 pixels per lane (tile size overrides)
        ngp_spoil_file(h, type);
        Q.L.fold[slot] = 0;
    }
    Q.L.sm_const[slot] = P.sm_const;
    Q.L.n = slot + 1;
    Q.particles += n * (uint64_t)(G.region / G.batch);  // bounds the records behind the pending chunks
    return SLICER_OK;
}

}  // namespace

int deposit_device_chunk(slicer_handle h, int type, const float *d_pos, const float *d_mass, uint64_t n)
{
    const slicer_plane_desc &d = h->desc;
    const bool has_mass = d_mass != nullptr;
    PassParams P;
    make_params(h, type, has_mass, P);
    Targets T;
    fill_targets(h, type, has_mass, T);
    const LaunchCfg cfg = launch_cfg(d, has_mass);
    if (d.snopt > 0)
        return thin_deposit_chunk(h, type, P, T, cfg, d_pos, d_mass, n);
    // One pass of the binned pipeline holds at most kMaxBins (plane, tile) bins and needs disjoint slabs.  A pass beyond
    // that (four 16384^2 planes; overlapping slabs) takes its planes in groups, each group a binned sub-pass over the
    // same chunk, before the fused global-atomic kernel is considered.
    int gsize = d.n_planes;
    BinGeom G;
    auto fits = [&](int p0, int np, BinGeom &Gs) {
        slicer_plane_desc sub = d;
        sub.n_planes = np;
        for (int j = 0; j < np; j++) {
            sub.ld[j] = d.ld[p0 + j];
            sub.ld2[j] = d.ld2[p0 + j];
            sub.nrepperp[j] = d.nrepperp[p0 + j];
        }
        return choose_geom(sub, cfg.acc, h->opt, Gs) && scatter_lds_bytes(Gs, has_mass) <= 160 * 1024 - 256;
    };
    bool binned = d.algo != SLICER_ALGO_DIRECT && fits(0, d.n_planes, G);
    if (!binned && d.algo != SLICER_ALGO_DIRECT)
        for (int g = d.n_planes - 1; g >= 1 && !binned; g--) {
            bool ok = true;
            for (int p0 = 0; p0 < d.n_planes && ok; p0 += g)
                ok = fits(p0, std::min(g, d.n_planes - p0), G);
            if (ok) {
                binned = true;
                gsize = g;
            }
        }
    if (!binned && d.algo == SLICER_ALGO_BINNED)
        return fail(h, SLICER_ERR_UNSUPPORTED,
                    "SLICER_ALGO_BINNED cannot serve this pass (a tile table beyond the limits even for a single "
                    "plane); SLICER_ALGO_AUTO falls back to the fused global-atomic kernel");
    if (binned && d.algo == SLICER_ALGO_AUTO && n < 65536)
        binned = false;  // several launches are not worth it for a tiny chunk
    h->algo_mask |= 1 << (binned ? SLICER_ALGO_BINNED : SLICER_ALGO_DIRECT);
    if (!binned) {
        if (d.mas == SLICER_MAS_NGP)
            ngp_spoil_file(h, type);  // counts into the global map
        ProfScope ps(h, KN_DIRECT);
        P.series_max = kSeriesMax15;  // no pre-test on this path: entries far outside the field reach project()
        HIPCHK(h, launch_direct(cfg, d_pos, d_mass, n, P, T, h->stream));
        return SLICER_OK;
    }
    for (int p0 = 0; p0 < d.n_planes; p0 += gsize) {
        const int np = std::min(gsize, d.n_planes - p0);
        PassParams Pg = P;
        Targets Tg = T;
        if (np != d.n_planes) {  // this group's planes move to the front
            fits(p0, np, G);
            planes_to_front(Pg, Tg, p0, np, true);
        }
        int nr = 0;
        for (int j = 0; j < np; j++)
            nr = std::max(nr, Pg.nrep[j]);
        const int nwin = rep_windows(nr), ws = rep_window_side(nr);
        for (int wi = 0; wi < nwin; wi++)
            for (int wj = 0; wj < nwin; wj++) {
                if (nwin > 1) {
                    Pg.rep_i0 = -nr + wi * ws;
                    Pg.rep_i1 = std::min(nr, Pg.rep_i0 + ws - 1);
                    Pg.rep_j0 = -nr + wj * ws;
                    Pg.rep_j1 = std::min(nr, Pg.rep_j0 + ws - 1);
                }
                int rc = binned_chunk(h, cfg, Pg, Tg, G, type, p0 / gsize, p0, np, d_pos, d_mass, n);
                if (rc)
                    return rc;
            }
    }
    return SLICER_OK;
}
