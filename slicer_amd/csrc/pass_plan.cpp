// pass_plan.cpp -- what a pass launches with: the uniform parameter block, the targets, the tile geometry of the binned
// path, the qualification of the fast project+bin kernel with its exhaustive device sweeps, and the slicer_debug_* entry
// points that expose them.
#include "slicer_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace slicer;

namespace {

float ceil_to_f32(double v)
{
    // smallest float >= v
    float f = (float)v;
    if ((double)f < v)
        f = std::nextafterf(f, INFINITY);
    return f;
}

constexpr int kUnitBins = 8192;   // up to this many bins the units are whole planes

int run_box_sweep(slicer_handle h, double box, unsigned out[9])
{
    if (!h->d_sweep)
        HIPCHK(h, hipMalloc((void **)&h->d_sweep, 9 * sizeof(unsigned)));
    HIPCHK(h, hipMemsetAsync(h->d_sweep, 0, 9 * sizeof(unsigned), h->stream));
    HIPCHK(h, launch_check_box_quotient(box, h->d_sweep, h->stream));
    out[0] = 1;
    HIPCHK(h, hipMemcpyAsync(out, h->d_sweep, 9 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SLICER_OK;
}

// Has the f32 form of r / box (k_project_bin_fast) been proven for this box size?  One exhaustive device sweep over
// all 2^31 non-negative floats per distinct box size and handle (a few milliseconds), then cached.
int box_quotient_ok(slicer_handle h, double box, bool &ok)
{
    for (auto &v : h->box_verdicts)
        if (v.first == box) {
            ok = v.second;
            return SLICER_OK;
        }
    unsigned out[9];
    int rc = run_box_sweep(h, box, out);
    if (rc)
        return rc;
    ok = out[0] == 0;
    h->box_verdicts.emplace_back(box, ok);
    return SLICER_OK;
}

}  // namespace

int acc_kind(const slicer_plane_desc &d, bool has_mass)
{
    if (d.mas == SLICER_MAS_NGP)
        return has_mass ? kF32 : kCountU32;
    switch (d.accum) {
    case SLICER_ACC_F64: return kF64;
    case SLICER_ACC_FIXED64: return kFixed64;
    default: return kF32;
    }
}

LaunchCfg launch_cfg(const slicer_plane_desc &d, bool has_mass)
{
    return LaunchCfg{d.mas == SLICER_MAS_NGP ? kNGP : kTSC, acc_kind(d, has_mass), has_mass};
}

// Build the uniform parameter block for (current file, type).
void make_params(slicer_handle h, int type, bool has_mass, PassParams &P)
{
    const slicer_plane_desc &d = h->desc;
    const slicer_file_desc &f = h->file;
    memset(&P, 0, sizeof P);
    P.box = f.boxsize;
    P.inv_box = 1.0 / f.boxsize;
    for (int a = 0; a < 3; a++) {
        P.c0[a] = f.center[a];
        P.sgn[a] = (float)f.sgn[a];
    }
    // gadget2io.cpp:222-252: face -> (x,y,z) = wrapped[perm]
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}, {1, 0, 2}, {2, 0, 1}, {2, 1, 0}};
    int fi = (f.face >= 1 && f.face <= 6) ? f.face - 1 : 0;  // any other value leaves case 1 (switch falls through)
    for (int a = 0; a < 3; a++) {
        P.perm[a] = perms[fi][a];
        for (int c = 0; c < 3; c++)
            P.pm[a][c] = perms[fi][a] == c ? 0xFFFFFFFFu : 0u;
    }
    P.rcase = f.rcase;
    P.n_planes = d.n_planes;
    for (int p = 0; p < d.n_planes; p++) {
        double minDist = d.ld[p] / f.boxsize * 1.e+3 / 1.0;   // densitymaps.cpp:346 (POS_U = 1.0)
        double maxDist = d.ld2[p] / f.boxsize * 1.e+3 / 1.0;  // densitymaps.cpp:347
        P.zlo[p] = ceil_to_f32(minDist);
        P.zhi[p] = ceil_to_f32(maxDist);
        P.nrep[p] = d.nrepperp[p];
    }
    for (int p = d.n_planes; p < kMaxPlanes; p++) {  // unused slots select nothing (kernels may unroll over all 8)
        P.zlo[p] = INFINITY;
        P.zhi[p] = -INFINITY;
    }
    P.rep_i0 = P.rep_j0 = -64;  // every lateral replica (the binned path narrows this per launch)
    P.rep_i1 = P.rep_j1 = 64;
    P.fov = d.fov_rad;
    P.inv_fov = 1.0 / d.fov_rad;
    P.lim = d.fov_rad * (1. + 2. / d.npix) * 0.5;  // densitymaps.cpp:383
    if (P.lim < 1.5) {
        P.tan_lim_hi = (float)(std::tan(P.lim) * (1.0 + 1e-5));
        P.sin2_lim_hi = (float)(std::sin(P.lim) * std::sin(P.lim) * (1.0 + 1e-5));
    }
    P.force_libm = d.debug_flags & 1;
    // every entry that reaches the series passed the f32 pre-test (|tan ra|, |sin dec| within 1e-5 of the limit's)
    // or, on the direct path, may lie anywhere: there, and with debug bit 1, keep the wide 15-term range
    P.series_max = (!(d.debug_flags & 2) && P.lim < 1.5 && std::tan(P.lim) * 1.001 < kSeriesMax9) ? kSeriesMax9
                                                                                                   : kSeriesMax15;
    P.nn = d.npix;
    P.pow2 = is_pow2(d.npix) ? 1 : 0;
    P.dl = 1. / double(d.npix);  // utilities.cpp:50
    P.nn_d = (double)d.npix;
    P.half_dl = 0.5 * P.dl;
    P.onehalf_dl = 0.5 * 3.0 * P.dl;
    P.dl_f = (float)P.dl;
    P.nn_f = (float)P.nn_d;
    P.half_dl_f = (float)P.half_dl;
    P.onehalf_dl_f = (float)P.onehalf_dl;
    auto round_down = [](double x) {
        float f = (float)x;
        return (double)f > x ? std::nextafterf(f, 0.0f) : f;
    };
    P.inv_dl = 1.0 / P.dl;
    P.dl_quot_ok = (!P.pow2 && h->dl_quot_ok) ? 1 : 0;
    P.half_dl_lo = round_down(P.half_dl);
    P.onehalf_dl_lo = round_down(P.onehalf_dl);
    P.mconst = (float)f.massarr[type];  // densitymaps.cpp:372
    P.sm_const = sqrtf(P.mconst);       // glibc sqrtf is correctly rounded, as std::sqrt(float)
    int e = d.want_type_maps ? h->fixed_exp[type] : h->fixed_exp_shared;
    P.fixed_scale = std::ldexp(1.0, e);
    {
        int le = 10;  // MAX_M = 1e3 < 2^10
        if (P.mconst > 0 && std::isfinite(P.mconst))
            le = std::ilogb(P.mconst) + 1;
        P.tile_scale = std::ldexp(1.0, 49 - le);
        P.tile_inv_scale = std::ldexp(1.0, le - 49);
        P.tile_cmin = std::ldexp(1.0f, le - 25);
    }
    (void)has_mass;
}

int pick_fixed_exp(const slicer_plane_desc &d, double m, bool has_mass)
{
    int frac = d.fixed_frac_bits > 0 ? d.fixed_frac_bits : 40;
    int le = 10;  // MAX_M = 1e3 < 2^10
    if (!has_mass && m > 0 && std::isfinite(m))
        le = std::ilogb(m) + 1;
    return frac - le;
}

void fill_targets(slicer_handle h, int type, bool has_mass, Targets &T)
{
    const slicer_plane_desc &d = h->desc;
    const int kind = acc_kind(d, has_mass);
    const bool ngp = d.mas == SLICER_MAS_NGP;
    const bool shared = !ngp && !d.want_type_maps;
    memset(&T, 0, sizeof T);
    for (int p = 0; p < d.n_planes; p++) {
        if (shared)
            T.acc[p] = h->planes[p].acc_shared.p;
        else if (ngp || kind != kF32)
            T.acc[p] = h->planes[p].acc[type].p;
        else
            T.acc[p] = h->planes[p].toti[type].p;
        T.nsel[p] = h->d_counts + (size_t)p * 6 + type;
    }
    T.neg_flag = h->d_neg;
    T.max_mass = h->d_maxmass + (shared ? 6 : type);
}

void planes_to_front(PassParams &P, Targets &T, int p0, int np, bool narrow)
{
    for (int j = 0; j < np; j++) {
        P.zlo[j] = P.zlo[p0 + j];
        P.zhi[j] = P.zhi[p0 + j];
        P.nrep[j] = P.nrep[p0 + j];
        T.acc[j] = T.acc[p0 + j];
        T.nsel[j] = T.nsel[p0 + j];
    }
    if (!narrow)
        return;
    P.n_planes = np;
    for (int j = np; j < kMaxPlanes; j++) {  // as make_params leaves the slots beyond the pass
        P.zlo[j] = INFINITY;
        P.zhi[j] = -INFINITY;
        P.nrep[j] = 0;
        T.acc[j] = nullptr;
        T.nsel[j] = nullptr;
    }
}

// Lateral replication (densitymaps.cpp:377-381): a pass with n replications per side has (2n+1)^2 replicas per particle.
// One launch of the binned project kernel takes a window of at most 7 x 7 of them; the side (2n+1) is cut into equal parts.
int rep_windows(int nrmax) { return (2 * nrmax + 1 + 6) / 7; }
int rep_window_side(int nrmax) { return (2 * nrmax + 1 + rep_windows(nrmax) - 1) / rep_windows(nrmax); }

// Tile geometry of the binned path.  Tiles are powers of two so that pixel -> tile is a shift.  4-byte
// LDS cells (NGP counts): up to 128 x 128 (+halo = 67.6 KiB of LDS, two workgroups per CU); 8-byte: 64 x 128.
// Small maps get smaller tiles so that the grid still has >= ~1024 workgroups.
bool choose_geom(const slicer_plane_desc &d, int acc, const Options &opt, BinGeom &G)
{
    int nrmax = 0;
    for (int p = 0; p < d.n_planes; p++)
        nrmax = std::max(nrmax, d.nrepperp[p]);
    // (2n+1)^2 records per particle must fit the 16-bit per-workgroup counters at a 1024-particle batch: beyond three
    // replications per side the replica grid is walked in windows of at most 7 x 7, one run of K1-K3 per window
    const int ws = rep_window_side(nrmax);
    const int reps = ws * ws;
    for (int p = 0; p < d.n_planes; p++)  // slabs must be disjoint: a particle enters at most one bin
        for (int q = p + 1; q < d.n_planes; q++)
            if (d.ld[p] < d.ld2[q] && d.ld[q] < d.ld2[p])
                return false;
    // tuning / test knobs of the handle (slicer_set_option)
    const int env_s = opt.tile_log2, env_h = opt.tile_h_log2;
    const int env_b = opt.bin_batch;
    const bool wide = acc != kCountU32;  // every mode but the NGP counts keeps 8-byte cells in LDS
    int s = 7;  // log2 tile side
    auto tiles = [&](int sl) {
        int tw = 1 << sl, th = 1 << (wide ? sl - 1 : sl);
        return (long)((d.npix + tw - 1) / tw) * (long)((d.npix + th - 1) / th);
    };
    while (s > 4 && tiles(s) * d.n_planes < 1024)
        s--;
    G.tw_log2 = s;
    G.th_log2 = wide ? s - 1 : s;
    if (env_s) {
        G.tw_log2 = env_s;
        G.th_log2 = env_h ? env_h : env_s;
    }
    G.ntx = (d.npix + (1 << G.tw_log2) - 1) >> G.tw_log2;
    G.nty = (d.npix + (1 << G.th_log2) - 1) >> G.th_log2;
    // units: whole planes while everything fits kUnitBins tiles, otherwise bands of tile rows (large maps)
    const int env_rows = opt.unit_rows;  // tests
    const long tiles_plane = (long)G.ntx * G.nty;
    if (tiles_plane * d.n_planes <= kUnitBins && !env_rows) {
        G.units_per_plane = 1;
        G.rows_per_unit = G.nty;
    } else {
        G.rows_per_unit = env_rows ? std::min(env_rows, G.nty) : std::max(1, 2048 / G.ntx);
        // at most kMaxUnits units per pass (a test override may ask for thinner bands than that allows)
        const int max_upp = std::max(1, kMaxUnits / d.n_planes);
        G.rows_per_unit = std::max(G.rows_per_unit, (G.nty + max_upp - 1) / max_upp);
        G.units_per_plane = (G.nty + G.rows_per_unit - 1) / G.rows_per_unit;
    }
    G.tiles_per_unit = G.rows_per_unit * G.ntx;
    G.n_units = d.n_planes * G.units_per_plane;
    const long nb = (long)G.n_units * G.tiles_per_unit;
    if (G.n_units > kMaxUnits || G.tiles_per_unit > 8192 || nb > kMaxBins)
        return false;
    G.nbins = (int)nb;
    // tuning overrides (tile_log2 / tile_h_log2 / bin_batch): the batch must keep every
    // workgroup's first particle 16-byte aligned (multiple of 4; kept at a multiple of 1024) and fit the 16-bit
    // per-workgroup counters
    G.batch = env_b ? std::min(std::max((env_b / 1024) * 1024, 1024), 64512) : kBinBatch;
    G.batch = std::min(G.batch, std::max(1024, 65535 / reps / 1024 * 1024));  // lateral replicas multiply the records
    G.region = G.batch * reps;
    if (G.tw_log2 < 3 || G.tw_log2 > 8 || G.th_log2 < 3 || G.th_log2 > 8)
        return false;
    return true;
}

// Maps that are not a power of two wide: may the grid arithmetic use quot_dl3 instead of f64 divisions by dl = 1/npix?
// One exhaustive device sweep (2^30 operands, ~1 ms) per distinct npix and handle, cached.  Option dl_quot = 0 says no.
int dl_quotient_ok(slicer_handle h, int npix, bool &ok, unsigned *examples9)
{
    if (!examples9)
        for (auto &v : h->dl_verdicts)
            if (v.first == npix) {
                ok = v.second;
                return SLICER_OK;
            }
    if (!h->d_sweep)
        HIPCHK(h, hipMalloc((void **)&h->d_sweep, 9 * sizeof(unsigned)));
    HIPCHK(h, hipMemsetAsync(h->d_sweep, 0, 9 * sizeof(unsigned), h->stream));
    HIPCHK(h, launch_check_dl_quotient(1. / double(npix), h->d_sweep, h->stream));
    unsigned out[9] = {1};
    HIPCHK(h, hipMemcpyAsync(out, h->d_sweep, sizeof out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ok = out[0] == 0;
    if (examples9)
        memcpy(examples9, out, sizeof out);
    else
        h->dl_verdicts.emplace_back(npix, ok);
    return SLICER_OK;
}

// Kernel arguments of k_project_bin_fast and whether this (file, pass) qualifies for it; see the conditions in
// slicer_project_bin.hip.  Option k1_general = 1 forces the general kernel (tests run both).
int k1_fast_args(slicer_handle h, const PassParams &P, const BinGeom &G, int nblocks, K1Args &A, bool &fast)
{
    memset(&A, 0, sizeof A);
    fast = false;
    if (h->opt.k1_general || P.n_planes > 4 || !(P.lim < 1.5) || G.region != G.batch ||
        (uint64_t)G.n_units * (uint64_t)nblocks * (uint64_t)G.region >= (1ull << 31))
        return SLICER_OK;
    for (int p = 0; p < P.n_planes; p++)
        if (P.nrep[p] != 0)
            return SLICER_OK;
    for (int p = 0; p + 1 < P.n_planes; p++)  // consecutive slabs (the planes of one box replication)
        if (!(P.zhi[p] == P.zlo[p + 1] && P.zlo[p] <= P.zhi[p]))
            return SLICER_OK;
    if (!(P.rcase >= 0.0f) || !std::isfinite(P.rcase) || !std::isfinite((float)P.box) || (float)P.box <= 0.0f)
        return SLICER_OK;
    for (int a = 0; a < 3; a++) {
        const double c = P.c0[a];
        // the recentring runs in f32: exact iff the centre is an f32 value (rand()/float(RAND_MAX) is one,
        // densitymaps.cpp:188-190)
        // (centres below 2^-20 -- e.g. the exact 0 of -DUSE_FIXED_PLC_VERTEX -- are where the reference's -0.0 and the
        // last bit of a quotient below 2^-100 could reach the result: left to the general kernel)
        if (!((double)(float)c == c) || !(c >= 0x1p-20 && c <= 1.0))
            return SLICER_OK;
    }
    bool ok = false;
    int rc = box_quotient_ok(h, P.box, ok);
    if (rc)
        return rc;
    if (!ok)
        return SLICER_OK;
    A.boxf = (float)P.box;
    A.rb = 1.0f / A.boxf;
    for (int a = 0; a < 3; a++) {
        const float sg = P.sgn[P.perm[a]];
        A.ws[a] = sg;
        A.wo[a] = sg < 0.0f ? 1.0f : 0.0f;
        A.c0f[a] = (float)P.c0[a];
    }
    static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}, {1, 0, 2}, {2, 0, 1}, {2, 1, 0}};
    A.face = 0;
    for (int f = 0; f < 6; f++)
        if (perms[f][0] == P.perm[0] && perms[f][1] == P.perm[1] && perms[f][2] == P.perm[2])
            A.face = f;
    A.rcase = P.rcase;
    A.n_planes = P.n_planes;
    {
        // expected fraction of particles that reach the projection: the slabs' share of the unit box depth
        // (positions are uniform in z to first order); option k1_stack = 0 / 1 overrides
        double depth = 0;
        for (int p = 0; p < P.n_planes; p++)
            depth += std::max(0.0, std::min<double>(P.zhi[p], P.rcase + 1.0) - std::max<double>(P.zlo[p], P.rcase));
        A.stack = h->opt.k1_stack >= 0 ? h->opt.k1_stack : (depth < 0.6 ? 1 : 0);
    }
    for (int p = 0; p < 4; p++)
        A.zlo[p] = P.zlo[p];  // +inf beyond n_planes (make_params)
    A.zlast = P.zhi[P.n_planes - 1];
    const double tl = std::tan(P.lim);
    A.k_ra = ceil_to_f32(tl * (1.0 + 3e-5));
    A.eps_ra = 2e-6f;
    A.k_dec = ceil_to_f32(tl * std::sqrt(1.0 + (double)A.k_ra * (double)A.k_ra) * (1.0 + 3e-5));
    A.eps_dec = ceil_to_f32(tl * 2.2e-6 + 1e-6);
    // both series of the fast kernel run on tangents: |tan ra| <= k_ra and |tan dec| = |X| / sqrt(Y^2 + Z^2) <= |X| / Z <=
    // k_dec (plus the pre-test's absolute slack) for every entry that passes the pre-test; entries beyond the chosen
    // range (15 terms: 0.3125) are left to the exact epilogue by the kernel
    A.series_max = (!(h->desc.debug_flags & 2) && (double)A.k_dec * 1.001 + 1e-4 < kSeriesMax9) ? kSeriesMax9 : kSeriesMax15;
    A.lim = P.lim;
    A.inv_fov = P.inv_fov;
    A.nn_f = P.nn_f;
    A.nn_d = P.nn_d;
    A.nn = P.nn;
    A.pow2 = P.pow2;
    fast = true;
    return SLICER_OK;
}

extern "C" {

int slicer_debug_project(slicer_handle h, int type, const float *d_pos, uint64_t n, float *d_xs, float *d_ys,
                         int32_t *d_plane, uint64_t *d_src, uint64_t capacity, uint64_t *n_out)
{
    int rc = check_deposit_args(h, type, d_pos, nullptr, n);
    if (rc)
        return rc;
    PassParams P;
    make_params(h, type, false, P);
    unsigned long long *d_count = nullptr;
    HIPCHK(h, hipMalloc((void **)&d_count, sizeof(unsigned long long)));
    HIPCHK(h, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), h->stream));
    {
        ProfScope ps(h, KN_DEBUG);
        HIPCHK(h, launch_debug_project(d_pos, n, P, d_xs, d_ys, d_plane, d_src, capacity, d_count, h->d_neg,
                                       h->stream));
    }
    unsigned long long c = 0;
    HIPCHK(h, hipMemcpyAsync(&c, d_count, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipFree(d_count));
    if (n_out)
        *n_out = c;
    return SLICER_OK;
}

int slicer_debug_box_quotient(slicer_handle h, double box, uint32_t *n_bad, uint32_t *examples8)
{
    if (!h || !n_bad)
        return fail(h, SLICER_ERR_ARG, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned out[9];
    int rc = run_box_sweep(h, box, out);
    if (rc)
        return rc;
    *n_bad = out[0];
    if (examples8)
        memcpy(examples8, out + 1, 8 * sizeof(uint32_t));
    return SLICER_OK;
}

int slicer_debug_dl_quotient(slicer_handle h, int32_t npix, uint32_t *n_bad, uint32_t *examples8)
{
    if (!h || !n_bad || npix < 1 || npix > 65536)
        return fail(h, SLICER_ERR_ARG, "slicer_debug_dl_quotient: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned out[9];
    bool ok;
    int rc = dl_quotient_ok(h, npix, ok, out);
    if (rc)
        return rc;
    *n_bad = out[0];
    if (examples8)
        memcpy(examples8, out + 1, 8 * sizeof(uint32_t));
    return SLICER_OK;
}

int slicer_debug_math(slicer_handle h, int op, const double *d_a, const double *d_b, double *d_out, uint64_t n)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (op < 0 || op > 11 || (n && (!d_a || !d_out || ((op == 1 || op >= 10) && !d_b))) || n > (1ull << 31))
        return fail(h, SLICER_ERR_ARG, "slicer_debug_math: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, launch_debug_math(op, d_a, d_b, d_out, n, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SLICER_OK;
}

}  // extern "C"
