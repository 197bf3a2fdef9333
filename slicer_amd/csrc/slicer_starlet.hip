// slicer_starlet.hip -- on-device starlet transform of a map (the isotropic undecimated wavelet transform, B3-spline
// a trous) and binned absolute sums, the starlet l1-norm.
//
// Starlet.  Of an n x n f32 map x (row-major, only read) and a scale count J: the index rule refl(i) mirrors about the
// edge pixels without repeating them (n = 1: 0; otherwise m = i mod 2 (n - 1) taken non-negative, refl = m < n ? m :
// 2 (n - 1) - m), as often as needed.  The line operator A_d along one axis, on f64 values v, step d = 2^j:
//   a = v[refl(i - d)] + v[refl(i + d)],  b = v[refl(i - 2 d)] + v[refl(i + 2 d)],  out[i] = (((6 v[i] + 4 a) + b) * 0.0625,
// every operation one IEEE f64 operation rounded once, no FMA (-ffp-contract=off).  c_0 = x widened exactly;
//   c_{j+1} = A_d along axis 0 of (A_d along axis 1 of c_j),  w_{j+1} = (float)(c_j - c_{j+1}),  coarse = (float)c_J,
// j = 0 ... J-1.  The c_j are f64 in global memory owned by the handle (two buffers, one read and one written by a
// level), never rounded to f32 between levels.
//
// k_starlet_level<TIn>: one launch a level (TIn = float for level 0, double after it).  It reads c_j once, writes c_{j+1}
// (not after the last level) and w_{j+1} (after the last level the coarse map too); the result of the row operator stays
// in registers.  The operator at step d couples pixels d apart only, so a tile is dilated: rows y0 + r d, r = 0 ...
// 2 seg - 1, and columns x0 + e + k d, e = 0 ... run - 1, k = 0 ... tc - 1: tc runs of `run` adjacent columns at stride d,
// 128 columns in all.  run = min(d, 16) (level_cfg): for d <= 16 the runs touch and the tile is a plain span of 128
// columns with a halo of 2 d a side; above that a run is 16 adjacent columns -- 128 B of an f64 row, 64 B of an f32 output
// row -- and the halo is two runs a side whatever d is.  The window, the tile and two more rows and runs on every side,
// is staged in LDS as f64 with the mirror index applied per element (a lane mirrors its three window columns once, a
// wave a row's index once a row; three rows of loads are in flight before the first store).  A thread owns one column of the tile and `seg` of its rows: it walks down the window, runs
// the row operator from LDS (five f64 reads at lane-adjacent addresses), keeps the last five results in registers and
// runs the column operator on them; the subtraction and both roundings are fused into the stores.  256 threads: 128
// columns x 2 row segments of at most 8 rows, so a window is 20 rows of 132 ... 192 f64: 21 ... 30 KiB, 7 ... 5 workgroups a CU.  The order of every output's operations is fixed above, so tile shapes change no bit.  No
// atomics; nothing is carried over between runs.
//
// l1-norm.  Of an n x n f32 map and N10's f64 edges e_0 < ... < e_B: per bin, by N10's PDF rule (x widened to f64, the
// last bin closed; below, above, nan), the int64 count and the f64 sum of |x|; below and above have sums too, NaN pixels
// enter none.
// k_l1norm: a workgroup is one wave.  The map is a flat array cut into chunks of 512 pixels, workgroup g of G takes
// chunks g, g + G, ... (G fixed by the handle: resident_groups), a lane pixels lane, lane + 64, ... of a chunk; the
// loads of its next chunk are in flight while it bins the current one.  The
// edges sit in LDS (rank_search and pdf_slot of slicer_rank_counts.hpp, N10's); counts are u32 in LDS (integer
// atomics).  The sums are C = 2^c copies of B + 2 f64 cells in LDS, lane l adds into copy l mod C, and the lanes of a
// wave take turns: in
// round r = 0 ... 64 / C - 1 the lanes with l / C = r add, plain read-add-write, no two of them into one cell.  So the
// order of every cell's additions is fixed by the pixel indices alone.  C is the largest power of two <= 64 whose
// copies fit in 32 KiB (64 bins: 32 copies, 2 rounds; 1024 bins: 2 copies, 32 rounds).  Flush: the copies of a cell
// are added in index order into row g of partial sums [G][B + 2], the counts stored as row g of [G][B + 3];
// k_column_sums<double, double> adds the rows of a column in a fixed order (sixteen threads take rows t, t + 16, ...,
// then thread 0 adds the sixteen in order), k_column_sums<unsigned, int64_t> the counts.  No floating-point atomics;
// every row and result is stored by every launch.  All terms are non-negative, so whatever the order
// |sum - S| <= (count - 1) 2^-53 S (1 + ...).
#include <hip/hip_runtime.h>

#include "slicer_rank_counts.hpp"

namespace {

constexpr int kMaxScales = SLICER_STARLET_MAX_SCALES;
constexpr int kLevelThreads = 256;
constexpr int kTileCols = 128;                         // columns of a tile = threads of a row segment
constexpr int kSegs = kLevelThreads / kTileCols;       // row segments of a tile
constexpr int kMaxSeg = 8, kMaxRunLog2 = 4;            // rows of a segment at most; log2 of the longest run
constexpr int kLaneCols = 3, kStageRows = 3;           // window columns a lane stages (the widest window is 192 columns); rows it loads before it stores

static_assert(kTileCols + (4 << kMaxRunLog2) <= 64 * kLaneCols, "three columns a lane cover the widest window");
static_assert((1 << (kMaxScales - 1)) * (2 * kMaxSeg + 4) + kMaxNpix < (1 << 30), "window indices before the mirror fit an int");

// refl(i) for any int i
__device__ __forceinline__ int mirror(int i, int n)
{
    if ((unsigned)i < (unsigned)n)
        return i;
    if (n == 1)
        return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0)
        m += p;
    return m < n ? m : p - m;
}

struct LevelArgs {
    const void *in;   // c_j: f32 (level 0) or f64
    double *next;     // c_{j+1}, or null after the last level
    float *w;         // w_{j+1}
    float *coarse;    // null but after the last level
    int n, d;
    int run_log2, seg;  // a run is 1 << run_log2 columns; a thread takes seg rows
    int pitch;          // window columns: kTileCols + 4 runs
    int res_r, kblocks_r, resblocks_c, kblocks_c;  // tiles: row residues x blocks of 2 seg rows x column residue runs x blocks of tc runs
};

template <class TIn>
__global__ __launch_bounds__(kLevelThreads) void k_starlet_level(LevelArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double win[];  // [rows][pitch]
    const int n = a.n, d = a.d, pitch = a.pitch, run = 1 << a.run_log2, tid = threadIdx.x;
    const int rows = kSegs * a.seg + 4;
    unsigned t = blockIdx.x;
    const int kcb = (int)(t % (unsigned)a.kblocks_c);
    t /= (unsigned)a.kblocks_c;
    const int ocb = (int)(t % (unsigned)a.resblocks_c);
    t /= (unsigned)a.resblocks_c;
    const int krb = (int)(t % (unsigned)a.kblocks_r), o_r = (int)(t / (unsigned)a.kblocks_r);
    const int y0 = o_r + krb * (kSegs * a.seg) * d;                          // window row wr = map row y0 + (wr - 2) d
    const int x0 = (ocb << a.run_log2) + kcb * (kTileCols >> a.run_log2) * d;  // window column wc = x0 + wc % run + (wc / run - 2) d
    // A wave stages whole window rows, a lane the window columns lane, lane + 64 and lane + 128 (pitch <= 192): their map
    // columns are mirrored once, a row's index once a row; three rows, nine loads, are in flight before the first store.
    const int lane = tid % 64;
    int mc[kLaneCols];
#pragma unroll
    for (int k = 0; k < kLaneCols; k++) {
        const int wc = lane + 64 * k;
        mc[k] = wc < pitch ? mirror(x0 + (wc & (run - 1)) + ((wc >> a.run_log2) - 2) * d, n) : 0;
    }
    const bool third = lane + 128 < pitch;  // (the first two columns always are in the window: pitch >= 132)
    const TIn *in = static_cast<const TIn *>(a.in);
    for (int wr0 = tid / 64; wr0 < rows; wr0 += kStageRows * (kLevelThreads / 64)) {
        TIn v[kStageRows][kLaneCols];
#pragma unroll
        for (int b = 0; b < kStageRows; b++) {  // (a row past the window: the last one again, loaded and not stored)
            const int wr = min(wr0 + b * (kLevelThreads / 64), rows - 1);
            const TIn *src = in + (size_t)mirror(y0 + (wr - 2) * d, n) * n;
#pragma unroll
            for (int k = 0; k < kLaneCols; k++)
                v[b][k] = src[mc[k]];
        }
#pragma unroll
        for (int b = 0; b < kStageRows; b++) {
            const int wr = wr0 + b * (kLevelThreads / 64);
            if (wr < rows) {  // (wave-uniform)
                double *dst = win + wr * pitch + lane;
                dst[0] = (double)v[b][0];
                dst[64] = (double)v[b][1];
                dst[third ? 128 : 0] = (double)(third ? v[b][2] : v[b][0]);  // (no branch: the third load stays with the others)
            }
        }
    }
    __syncthreads();
    const int cw = tid % kTileCols, sg = tid / kTileCols;
    const int col = x0 + (cw & (run - 1)) + (cw >> a.run_log2) * d;
    if (col >= n)
        return;
    const double *base = win + cw + 2 * run;  // the thread's column of the window
    const auto rowop = [base, pitch, run](int wr) {
        const double *p = base + wr * pitch;
        const double s1 = p[-run] + p[run];
        const double s2 = p[-2 * run] + p[2 * run];
        return ((6.0 * p[0] + 4.0 * s1) + s2) * 0.0625;
    };
    const int wr0 = sg * a.seg;  // window rows wr0 ... wr0 + seg + 3 are under the outputs of window rows wr0 + 2 ...
    double r0 = rowop(wr0), r1 = rowop(wr0 + 1), r2 = rowop(wr0 + 2), r3 = rowop(wr0 + 3);
    for (int i = 0; i < a.seg; i++) {
        const int row = y0 + (wr0 + i) * d;
        if (row >= n)
            break;
        const double r4 = rowop(wr0 + i + 4);
        const double s1 = r1 + r3;
        const double s2 = r0 + r4;
        const double cn = ((6.0 * r2 + 4.0 * s1) + s2) * 0.0625;
        const double cj = base[(wr0 + i + 2) * pitch];
        const size_t at = (size_t)row * n + col;
        a.w[at] = (float)(cj - cn);
        if (a.next)
            a.next[at] = cn;
        if (a.coarse)
            a.coarse[at] = (float)cn;
        r0 = r1, r1 = r2, r2 = r3, r3 = r4;
    }
}

struct LevelCfg {
    int run_log2 = 0, seg = 1;
    int pitch = 0, res_r = 0, kblocks_r = 0, resblocks_c = 0, kblocks_c = 0;
    size_t lds = 0;
    unsigned grid = 0;
};

// The tile of level j for a map of n: runs of min(d, 16) columns (a plain span up to d = 16, dilated above), segments of
// 8 rows (measured against 16 and 4: DESIGN.md), fewer where a row residue has fewer than 16 rows.
LevelCfg level_cfg(int n, int j)
{
    LevelCfg c;
    const int d = 1 << j;
    c.run_log2 = std::min(j, kMaxRunLog2);
    const int per_residue = (n + d - 1) / d;  // rows (columns) y with y mod d = o, at most
    c.seg = std::max(1, std::min(kMaxSeg, (per_residue + kSegs - 1) / kSegs));
    c.pitch = kTileCols + (4 << c.run_log2);
    const int tc = kTileCols >> c.run_log2, run = 1 << c.run_log2;
    c.res_r = std::min(d, n);
    c.kblocks_r = (per_residue + kSegs * c.seg - 1) / (kSegs * c.seg);
    c.resblocks_c = (std::min(d, n) + run - 1) / run;
    c.kblocks_c = (per_residue + tc - 1) / tc;
    const int rows = kSegs * c.seg + 4;
    c.lds = (size_t)rows * c.pitch * sizeof(double);
    c.grid = (unsigned)((uint64_t)c.res_r * c.kblocks_r * c.resblocks_c * c.kblocks_c);  // < 2^23 for n <= 131072
    return c;
}

// ---- l1-norm ----
constexpr int kL1Threads = 64, kL1Per = 8;
constexpr int kL1Chunk = kL1Threads * kL1Per;
constexpr size_t kL1CopyBytes = 32 * 1024;  // the copies of the sums in LDS, at most

static_assert(((uint64_t)kMaxNpix * kMaxNpix / kMinGroups) < ((uint64_t)1 << 32), "a workgroup's u32 counters hold every pixel it can meet");

struct L1Args {
    const float *x;
    const double *edges;  // [B + 1]
    double *psum;         // [gridDim.x][B + 2]
    unsigned *pcnt;       // [gridDim.x][B + 3]
    uint64_t npixels, nchunks;
    int B, copies_log2;
};

__global__ __launch_bounds__(kL1Threads) void k_l1norm(L1Args a)
{
    extern __shared__ double dyn[];
    const int B = a.B, nS = B + 2, nC = B + 3, cl = a.copies_log2, lane = threadIdx.x;
    double *edge = dyn;                // [B + 1]
    double *acc = dyn + (B + 1);       // [B + 2][1 << cl]: slot B is below, B + 1 above
    unsigned *cnt = reinterpret_cast<unsigned *>(acc + ((size_t)nS << cl));  // [B + 3]: ... and B + 2 the NaNs
    stage_table<kL1Threads>(edge, a.edges, B + 1);
    for (int k = lane; k < nS << cl; k += kL1Threads)
        acc[k] = 0.0;
    for (int k = lane; k < nC; k += kL1Threads)
        cnt[k] = 0u;
    __syncthreads();
    const double eB = edge[B];
    const int copy = lane & ((1 << cl) - 1), my_round = lane >> cl, rounds = kL1Threads >> cl;
    volatile double *cells = acc;  // (every access is made: the rounds below are not merged)
    // the loads of a workgroup's next chunk are in flight while it bins the current one
    const auto load = [&a, lane](uint64_t chunk, float (&v)[kL1Per]) {
        const uint64_t first = chunk * kL1Chunk + (uint64_t)lane;
#pragma unroll
        for (int q = 0; q < kL1Per; q++) {
            const uint64_t p = first + (uint64_t)(q * kL1Threads);
            v[q] = chunk < a.nchunks && p < a.npixels ? a.x[p] : 0.0f;
        }
    };
    float cur[kL1Per], nxt[kL1Per];
    load(blockIdx.x, cur);
    for (uint64_t chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
        load(chunk + gridDim.x, nxt);
        const uint64_t first = chunk * kL1Chunk + (uint64_t)lane;
        double xd[kL1Per];
        bool in[kL1Per];
        int pos[kL1Per];
#pragma unroll
        for (int q = 0; q < kL1Per; q++) {
            in[q] = first + (uint64_t)(q * kL1Threads) < a.npixels;
            xd[q] = (double)cur[q];
        }
        rank_search(edge, B, xd, pos);
#pragma unroll
        for (int q = 0; q < kL1Per; q++) {
            const double x = xd[q];
            const int slot = pdf_slot(x, pos[q], eB, B, 1);  // a bin, or B: below, B + 1: above, B + 2: NaN
            if (in[q])
                atomicAdd(&cnt[slot], 1u);
            const bool adds = in[q] && slot < nS;
            const double mag = fabs(x);
            for (int r = 0; r < rounds; r++) {
                if (adds && my_round == r) {
                    const int cell = (slot << cl) + copy;
                    cells[cell] = cells[cell] + mag;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
#pragma unroll
        for (int q = 0; q < kL1Per; q++)
            cur[q] = nxt[q];
    }
    __syncthreads();
    for (int s = lane; s < nS; s += kL1Threads)
        a.psum[(size_t)blockIdx.x * nS + s] = fold_copies(acc, s, cl);
    for (int k = lane; k < nC; k += kL1Threads)
        a.pcnt[(size_t)blockIdx.x * nC + k] = cnt[k];
}

int l1_copies_log2(int B) { return lg_copies((size_t)(B + 2) * sizeof(double), kL1CopyBytes, 6); }

size_t l1_lds(int B, int cl)
{
    return (size_t)(B + 1) * sizeof(double) + (((size_t)(B + 2) * sizeof(double)) << cl) + (size_t)(B + 3) * sizeof(unsigned);
}

// H_j as integers over 16^j, j = 0 ... J: H_0 = (1), H_j = H_{j-1} * (1, 4, 6, 4, 1) dilated by 2^{j-1}; centred, odd lengths
std::vector<std::vector<uint64_t>> starlet_tables(int J)
{
    std::vector<std::vector<uint64_t>> H(J + 1);
    H[0] = {1};
    static const uint64_t tap[5] = {1, 4, 6, 4, 1};
    for (int j = 1; j <= J; j++) {
        const size_t d = (size_t)1 << (j - 1);
        H[j].assign(H[j - 1].size() + 4 * d, 0);
        for (size_t k = 0; k < H[j - 1].size(); k++)
            for (int t = 0; t < 5; t++)
                H[j][k + t * d] += H[j - 1][k] * tap[t];
    }
    return H;
}

const RankModule kL1Norm = {"slicer_l1norm", "slicer_l1norm_create", "edges", "fewer than 2 edges", 2, SLICER_PEAKS_MAX_BINS + 1,
                            kMaxNpix};

}  // namespace

struct slicer_starlet : SubHandle {
    int n = 0, J = 0;
    float *out = nullptr;                // [J + 1][n^2] of the handle's n: the coarse map, then w_1 ... w_J
    double *c[2] = {nullptr, nullptr};   // c_j in c[j % 2] for j >= 1
    int ran_n = 0;                       // npix of the last run, 0 before any
};

struct slicer_l1norm : RankHandle {  // table: the B + 1 edges
    int B = 0, copies_log2 = 0;
    double *psum = nullptr, *sums = nullptr;
    unsigned *pcnt = nullptr;
    int64_t *counts = nullptr;
};

extern "C" {

int slicer_starlet_gains(int32_t scales, double *gain_w, double *gain_coarse)
{
    if (scales < 1 || scales > kMaxScales)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_starlet_gains: scales = %d outside 1..%d", scales, kMaxScales);
    // With P = 16 H_{j-1} and Q = H_j over 16^j, both centred on one support: sum_ab (P_a P_b - Q_a Q_b)^2 =
    // (sum P^2)^2 - 2 (sum P Q)^2 + (sum Q^2)^2.  The three sums are exact integers below 2^98; the rest is long double.
    const auto H = starlet_tables(scales);
    for (int j = 1; j <= scales; j++) {
        const std::vector<uint64_t> &P = H[j - 1], &Q = H[j];
        const size_t shift = (Q.size() - P.size()) / 2;
        unsigned __int128 pp = 0, pq = 0, qq = 0;
        for (size_t k = 0; k < Q.size(); k++)
            qq += (unsigned __int128)Q[k] * Q[k];
        for (size_t k = 0; k < P.size(); k++) {
            pp += (unsigned __int128)(16 * P[k]) * (16 * P[k]);
            pq += (unsigned __int128)(16 * P[k]) * Q[k + shift];
        }
        const long double unit = ldexpl(1.0L, -8 * j);  // 1 / (16^j)^2
        const long double spp = (long double)pp * unit, spq = (long double)pq * unit, sqq = (long double)qq * unit;
        if (gain_w)
            gain_w[j - 1] = (double)sqrtl((spp * spp - 2.0L * (spq * spq)) + sqq * sqq);
        if (j == scales && gain_coarse)
            *gain_coarse = (double)sqq;  // sqrt(sum_ab (Q_a Q_b)^2) = sum Q^2
    }
    return SLICER_OK;
}

int slicer_starlet_create(slicer_handle h, int32_t npix, int32_t scales, slicer_starlet_handle *out)
{
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    const char *who = "slicer_starlet_create";
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, who, npix, kMaxNpix))
        return rc;
    if (scales < 1 || scales > kMaxScales)
        return fail(h, SLICER_ERR_ARG, "%s: scales = %d outside 1..%d", who, scales, kMaxScales);
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    hipStream_t st = nullptr;
    slicer_starlet_handle sh = nullptr;
    if (int rc = sub_new(h, who, &st, &sh))
        return rc;
    sh->n = npix;
    sh->J = scales;
    const size_t np2 = (size_t)npix * (size_t)npix;
    int rc = SLICER_OK;
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->out, (size_t)(scales + 1) * np2 * sizeof(float));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->c[0], np2 * sizeof(double));
    rc = sh->mem.alloc(rc, h, who, (void **)&sh->c[1], np2 * sizeof(double));
    return sub_done(rc, sh, out);
}

int slicer_starlet_run_npix(slicer_starlet_handle sh, const float *d_map, int32_t npix)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_starlet_run_npix: null argument");
    if (npix < 1 || npix > sh->n)
        return fail(sh->h, SLICER_ERR_ARG, "slicer_starlet_run_npix: npix = %d outside 1..%d", npix, sh->n);
    const size_t np2 = (size_t)npix * (size_t)npix, own = (size_t)sh->n * (size_t)sh->n;
    if (ranges_overlap(d_map, np2 * sizeof(float), sh->out, (size_t)(sh->J + 1) * own * sizeof(float)) ||
        ranges_overlap(d_map, np2 * sizeof(float), sh->c[0], own * sizeof(double)) ||
        ranges_overlap(d_map, np2 * sizeof(float), sh->c[1], own * sizeof(double)))
        return fail(sh->h, SLICER_ERR_ARG, "slicer_starlet_run_npix: the input overlaps the handle's own buffers");
    hipStream_t st;
    if (int rc = sub_stream(sh->h, sh->device, &st))
        return rc;
    sh->ran_n = 0;
    for (int j = 0; j < sh->J; j++) {
        const LevelCfg c = level_cfg(npix, j);
        const bool last = j == sh->J - 1;
        LevelArgs a{};
        a.in = j == 0 ? (const void *)d_map : (const void *)sh->c[j % 2];
        a.next = last ? nullptr : sh->c[(j + 1) % 2];
        a.w = sh->out + (size_t)(j + 1) * own;
        a.coarse = last ? sh->out : nullptr;
        a.n = npix;
        a.d = 1 << j;
        a.run_log2 = c.run_log2;
        a.seg = c.seg;
        a.pitch = c.pitch;
        a.res_r = c.res_r;
        a.kblocks_r = c.kblocks_r;
        a.resblocks_c = c.resblocks_c;
        a.kblocks_c = c.kblocks_c;
        // (three names for three kinds of traffic: f32 in, f64 in and out, no f64 out; one level alone is the first)
        ProfScope ps(sh->h, j == 0 ? KN_STARLET_FIRST : last ? KN_STARLET_LAST : KN_STARLET_LEVEL);
        if (j == 0)
            hipLaunchKernelGGL(k_starlet_level<float>, dim3(c.grid), dim3(kLevelThreads), c.lds, st, a);
        else
            hipLaunchKernelGGL(k_starlet_level<double>, dim3(c.grid), dim3(kLevelThreads), c.lds, st, a);
        HIPCHK(sh->h, hipGetLastError());
    }
    sh->ran_n = npix;
    return SLICER_OK;
}

int slicer_starlet_run(slicer_starlet_handle sh, const float *d_map)
{
    if (!sh || !d_map)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_starlet_run: null argument");
    return slicer_starlet_run_npix(sh, d_map, sh->n);
}

int slicer_starlet_device_map(slicer_starlet_handle sh, int32_t scale, float **d_out)
{
    if (!sh || !d_out)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_starlet_device_map: null argument");
    if (scale < 0 || scale > sh->J)
        return fail(sh->h, SLICER_ERR_ARG, "slicer_starlet_device_map: scale = %d outside 0..%d", scale, sh->J);
    if (!sh->ran_n)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_starlet_device_map before any slicer_starlet_run");
    *d_out = sh->out + (size_t)scale * (size_t)sh->n * (size_t)sh->n;
    return SLICER_OK;
}

int slicer_starlet_read(slicer_starlet_handle sh, int32_t scale, float *host)
{
    if (!sh || !host)
        return fail(sh ? sh->h : nullptr, SLICER_ERR_ARG, "slicer_starlet_read: null argument");
    if (scale < 0 || scale > sh->J)
        return fail(sh->h, SLICER_ERR_ARG, "slicer_starlet_read: scale = %d outside 0..%d", scale, sh->J);
    if (!sh->ran_n)
        return fail(sh->h, SLICER_ERR_STATE, "slicer_starlet_read before any slicer_starlet_run");
    return sub_read(*sh, host, sh->out + (size_t)scale * (size_t)sh->n * (size_t)sh->n,
                    (size_t)sh->ran_n * (size_t)sh->ran_n * sizeof(float));
}

int slicer_starlet_destroy(slicer_starlet_handle sh) { return sub_destroy(sh); }

int slicer_l1norm_create(slicer_handle h, int32_t npix, int32_t n_edges, const double *edges, slicer_l1norm_handle *out)
{
    hipStream_t st = nullptr;
    slicer_l1norm_handle lh = nullptr;
    int rc = rank_create(h, kL1Norm, npix, n_edges, edges, out, &st, &lh);
    if (!lh)
        return rc;
    const char *who = kL1Norm.create;
    lh->B = n_edges - 1;
    lh->copies_log2 = l1_copies_log2(lh->B);
    const uint64_t np2 = (uint64_t)npix * (uint64_t)npix;
    lh->gmax = resident_groups(l1_lds(lh->B, lh->copies_log2), (int64_t)((np2 + kL1Chunk - 1) / kL1Chunk), h->num_cus);
    const size_t nS = (size_t)lh->B + 2, nC = (size_t)lh->B + 3;
    rc = lh->mem.alloc(rc, h, who, (void **)&lh->psum, (size_t)lh->gmax * nS * sizeof(double));
    rc = lh->mem.alloc(rc, h, who, (void **)&lh->pcnt, (size_t)lh->gmax * nC * sizeof(unsigned));
    rc = lh->mem.alloc(rc, h, who, (void **)&lh->sums, nS * sizeof(double));
    rc = lh->mem.alloc(rc, h, who, (void **)&lh->counts, nC * sizeof(int64_t));
    return sub_done(rank_upload(rc, *lh, kL1Norm, st), lh, out);
}

int slicer_l1norm_run_npix(slicer_l1norm_handle lh, const float *d_map, int32_t npix)
{
    hipStream_t st;
    if (int rc = rank_run_begin(lh, d_map, npix, kL1Norm, &st))
        return rc;
    const int nS = lh->B + 2, nC = lh->B + 3;
    L1Args a{};
    a.x = d_map;
    a.edges = lh->d_table;
    a.psum = lh->psum;
    a.pcnt = lh->pcnt;
    a.npixels = (uint64_t)npix * (uint64_t)npix;
    a.nchunks = (a.npixels + kL1Chunk - 1) / kL1Chunk;
    a.B = lh->B;
    a.copies_log2 = lh->copies_log2;
    const int G = (int)std::min<uint64_t>(a.nchunks, (uint64_t)lh->gmax);
    {
        ProfScope ps(lh->h, KN_L1NORM);
        hipLaunchKernelGGL(k_l1norm, dim3((unsigned)G), dim3(kL1Threads), l1_lds(lh->B, lh->copies_log2), st, a);
        HIPCHK(lh->h, hipGetLastError());
    }
    {
        ProfScope ps(lh->h, KN_L1NORM_FINISH);
        launch_column_sums(st, lh->psum, G, nS, lh->sums);
        launch_column_sums(st, lh->pcnt, G, nC, lh->counts);
        HIPCHK(lh->h, hipGetLastError());
    }
    lh->ran = true;
    return SLICER_OK;
}

int slicer_l1norm_run(slicer_l1norm_handle lh, const float *d_map)
{
    if (int rc = rank_not_null(lh, d_map, kL1Norm, ""))
        return rc;
    return slicer_l1norm_run_npix(lh, d_map, lh->n);
}

int slicer_l1norm_read(slicer_l1norm_handle lh, int64_t *counts, double *sums, int64_t *below, int64_t *above,
                       int64_t *n_nan, double *below_sum, double *above_sum)
{
    if (int rc = rank_read_begin(lh, kL1Norm))
        return rc;
    const size_t B = (size_t)lh->B;
    if (int rc = read_slices(*lh, lh->counts, {{counts, B}, {below, 1}, {above, 1}, {n_nan, 1}}))
        return rc;
    std::vector<double> s(B + 2);
    if (int rc = sub_read(*lh, s.data(), lh->sums, s.size() * sizeof(double)))
        return rc;
    if (sums)
        std::copy_n(s.data(), B, sums);
    if (below_sum)
        *below_sum = s[B];
    if (above_sum)
        *above_sum = s[B + 1];
    return SLICER_OK;
}

int slicer_l1norm_destroy(slicer_l1norm_handle lh) { return sub_destroy(lh); }

}  // extern "C"
