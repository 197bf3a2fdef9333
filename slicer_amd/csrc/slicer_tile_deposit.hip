// slicer_tile_deposit.hip -- SLICER_ALGO_BINNED, K4: the work-item builder and the LDS-privatised tile deposit
// (overview of the path: slicer_binned_common.hpp).
#include "slicer_binned_common.hpp"

#pragma clang fp contract(off)

namespace slicer {

// ---------------------------------------------------------------------------------------------
// K4: LDS-privatised tile deposit
// ---------------------------------------------------------------------------------------------
// Global accumulator type of each mode, and the type of the LDS tile cell.  Measured on MI355X
// (tools/lds_atomic_bench.hip, 3x3 random cells of a 130x130 tile, 512-thread workgroups):
//   ds_add_f32 0.20 T lane-ops/s   ds_add_f64 1.81 T   ds_add_u64 3.51 T   ds_add_u32 6.61 T
// ds_add_f32 is 9x slower than ds_add_f64, so no mode keeps f32 cells in LDS: f32/f64 modes sum the
// tile in f64 (and round once per flush), fixed point in u64, NGP counts in u32.
template <int ACC> struct AccT { using type = float; using lds = double; };
template <> struct AccT<kF64> { using type = double; using lds = double; };
template <> struct AccT<kFixed64> { using type = unsigned long long; using lds = unsigned long long; };
template <> struct AccT<kCountU32> { using type = unsigned; using lds = unsigned; };
template <> struct AccT<kF32I> { using type = float; using lds = unsigned long long; };
template <> struct AccT<kF64I> { using type = double; using lds = unsigned long long; };
template <int ACC> constexpr bool kIntCells = ACC == kF32I || ACC == kF64I;

// Integer tile cells of the F32 / F64 modes.  A contribution c is exact in units of 2^-49 of the mass scale iff
// c * tile_scale is an integer -- true for every c >= tile_cmin = 2^-25 scales (24-bit mantissa), i.e. for all but the
// ~0.1 % of contributions that are vanishing TSC weights.  Those are not rounded into the tile (a pixel holding nothing
// else must come out exact: T-TSC with k = 1) but added straight to the global map with a float atomic.  The kernel
// tests one number per record -- the smallest of its nine products -- and notes the rare records that fail in an LDS
// list, treated after the loop (slow_record); the loop itself stays branch-free.
constexpr unsigned kSlowCap = 512;  // noted records per work item (<= 16384 records: 1 % are ~160)

// The quantum of an integer-cell tile: 2^(le - 49) with 2^le above the (largest) particle mass of the launch.  With one
// constant mass it comes from the pass parameters; with per-particle masses from the largest selected mass the sort
// kernel has seen for the species (Targets::max_mass), read when the tile kernel starts.
struct TileQuantum {
    double scale, inv_scale;  // 2^(49 - le), 2^(le - 49)
    float cmin;               // 2^(le - 25): every contribution >= this is an exact multiple of the quantum
};

// HAS_MASS: the contribution carries a per-particle mass, which may be NaN or negative (sqrt -> NaN).  The f64 cells
// carry such a NaN to the map as the reference does; the FIXED64 accumulator cannot hold one, so there a contribution
// that is not finite adds nothing (include/slicer_amd.h, "hostile input").  Constant masses are checked on the host
// (slicer_file_begin): those instantiations have no test here.
template <int ACC, bool HAS_MASS>
__device__ __forceinline__ void lds_add(typename AccT<ACC>::lds *cell, float c, const PassParams &P, const TileQuantum &Q)
{
    if (ACC == kF32 || ACC == kF64) {
        atomicAdd(reinterpret_cast<double *>(cell), (double)c);  // ds_add_f64
    } else if (ACC == kFixed64) {
        if (HAS_MASS && !contribution_finite(c))
            return;
        atomicAdd(reinterpret_cast<unsigned long long *>(cell), rn_scaled_u64(c, P.fixed_scale));  // ds_add_u64
    }
    else if (kIntCells<ACC>)
        atomicAdd(reinterpret_cast<unsigned long long *>(cell), rn_scaled_u64(c, Q.scale));
}

// One record of an integer-cell tile with the representability test per contribution: exact ones into the tile, the
// others straight to the global accumulator map (gmap, acc_t = float or double).
template <int ACC, bool POW2>
__device__ __forceinline__ void slow_record(float xs, float ys, float sq, const PassParams &P, const TileQuantum &Q,
                                            typename AccT<ACC>::lds *tile, typename AccT<ACC>::type *gmap, int x0, int y0,
                                            int W)
{
    using acc_t = typename AccT<ACC>::type;
    const int nn = P.nn;
    const int gx = grid_index<POW2>(xs, P), gy = grid_index<POW2>(ys, P);
    float wx[3], wy[3];
    tsc_axis<POW2>(xs, gx, P, wx);
    tsc_axis<POW2>(ys, gy, P, wy);
    for (int a = 0; a < 3; a++) {
        wx[a] = sq * wx[a];
        wy[a] = sq * wy[a];
    }
    for (int b = 0; b < 3; b++)
        for (int a = 0; a < 3; a++) {
            const int px = gx + a - 1, py = gy + b - 1;
            if (px < 0 || px >= nn || py < 0 || py >= nn)
                continue;
            const float c = wx[a] * wy[b];
            const double t = (double)c * Q.scale;
            if (t == rint(t))
                atomicAdd(reinterpret_cast<unsigned long long *>(tile + (gy - y0 + b) * W + (gx - x0 + a)),
                          (unsigned long long)t);
            else
                atomicAdd(gmap + (size_t)px + (size_t)nn * (size_t)py, (acc_t)c);
        }
}

// Work items of the tile kernel: a (plane, tile) bin with many records (a halo core can put 10^5..10^7
// particles into one tile) is split into parts of <= kItemRecs records, each deposited by its own workgroup
// into its own LDS tile and flushed atomically, so that one heavy tile neither serialises on one CU nor
// stretches the kernel's tail.  Empty bins get no item.
#ifndef SLICER_ITEM_RECS
#define SLICER_ITEM_RECS 16384
#endif
constexpr unsigned kItemRecs = SLICER_ITEM_RECS;
#ifndef SLICER_WHOLE_RECS
#define SLICER_WHOLE_RECS 65536
#endif
// ... but a bin of up to kWholeRecs records stays whole: every part pays for zeroing and flushing a tile of its own
// (536 us against 554 us for the uniform headline case), while only a bin far beyond the usual load needs many hands
constexpr unsigned kWholeRecs = SLICER_WHOLE_RECS;
// Integer cells (kF32I / kF64I) count units of 2^(le - 49) with 2^le above the mass: one contribution is below
// 0.5625 * 2^49 units (TSC centre weight 0.75^2), so the N records a single workgroup may add to one u64 cell must keep
// N * 0.5625 * 2^49 < 2^64, i.e. N <= 58254.  A launch with integer cells therefore keeps a bin whole only up to
// kWholeRecsInt records; parts of split bins hold <= kItemRecs.  (f64, fixed-point -- 2^9 times the room -- and count
// cells keep kWholeRecs.)
#ifndef SLICER_WHOLE_RECS_INT
#define SLICER_WHOLE_RECS_INT 32768
#endif
constexpr unsigned kWholeRecsInt = SLICER_WHOLE_RECS_INT;
static_assert(SLICER_ITEM_RECS <= 58254, "a part must fit the integer cells' headroom");
#ifndef SLICER_MERGE_RECS
#define SLICER_MERGE_RECS 131072
#endif
// bins beyond about SLICER_MERGE_RECS records (a halo core) go through the wave-level pre-reduction
constexpr unsigned kMergeParts = SLICER_MERGE_RECS / kItemRecs > 2 ? SLICER_MERGE_RECS / kItemRecs : 2;

struct TileItems {
    unsigned *nparts;   // [nbins] parts of every bin (0 = empty: no work item)
    uint2 *extra;       // {bin, part} of the parts >= 1 of heavy bins, in no particular order
    unsigned *n_extra;  // entries of extra[]: zero before k_build_items, which also zeroes next_n_extra
    unsigned *next_n_extra;
};

// Work items of the tile kernel: part 0 of bin b is workgroup b; the further parts of heavy bins are appended to a
// list with one atomic add per heavy bin (their order does not matter), so that the builder is a plain parallel
// kernel instead of a single-workgroup scan.
__global__ __launch_bounds__(256) void k_build_items(PendingList L, int nbins, TileItems I, int whole, unsigned whole_recs)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b == 0)
        *I.next_n_extra = 0;  // the counter of the next launch (stream order makes this safe)
    if (b >= nbins)
        return;
    unsigned tot = 0;
    if (L.tot) {  // two-level sort: the sort kernel summed every pending chunk's records of the bin; zeroed for the next list
        tot = L.tot[b];
        L.tot[b] = 0;
    } else {
        for (int c = 0; c < L.n; c++)
            tot += L.base[c][b + 1] - L.base[c][b];
    }
    // (whole: the launch folds NGP counts file by file inside the tile kernel, which needs every tile in one workgroup)
    const unsigned np = (whole || tot <= whole_recs) ? (tot != 0) : (tot + kItemRecs - 1) / kItemRecs;
    I.nparts[b] = np;
    if (np > 1) {
        const unsigned at = atomicAdd(I.n_extra, np - 1);
        for (unsigned q = 1; q < np; q++)
            I.extra[at + q - 1] = make_uint2((unsigned)b, q);
    }
}

constexpr int kTileBlock = 1024;

// What both walkers below do with one record (xs, ys) of the tile: record index `i` of pending chunk `c`, with the
// chunk's constant mass and its root {mconst, sm_const}, or (HAS_MASS) its own raw mass `mraw`.  The NGP cell add, or the
// nine TSC additions.  CHECK = false for tiles whose halo lies inside the map (all but the border tiles): the per-cell
// map-edge tests and their exec-mask bookkeeping go.  The walkers load the record themselves (clamped, unconditional).
template <int MAS, int ACC, bool POW2, bool HAS_MASS, bool CHECK>
__device__ __forceinline__ void deposit_record(float xs, float ys, float mraw, float mconst, float sm_const, unsigned c,
                                               unsigned i, const PassParams &P, const TileQuantum &Q,
                                               typename AccT<ACC>::lds *tile, typename AccT<ACC>::type *gmap, int x0,
                                               int y0, int W, unsigned *s_nslow, uint2 *s_slow)
{
    using lds_t = typename AccT<ACC>::lds;
    const int nn = P.nn;
    float m = mconst, sq = sm_const;
    if (HAS_MASS) {
        m = cap_mass(mraw);
        sq = sqrt_mass(m);
    }
    const int gx = grid_index<POW2>(xs, P);
    const int gy = grid_index<POW2>(ys, P);
    if (MAS == kNGP) {
        lds_t *cell = tile + (gy - y0 + 1) * W + (gx - x0 + 1);
        if (ACC == kCountU32)
            atomicAdd(reinterpret_cast<unsigned *>(cell), 1u);
        else
            atomicAdd(reinterpret_cast<double *>(cell), (double)m);
    } else {
        float wx[3], wy[3];
        tsc_axis<POW2>(xs, gx, P, wx);
        tsc_axis<POW2>(ys, gy, P, wy);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            wx[a] = sq * wx[a];
            wy[a] = sq * wy[a];
        }
        if (kIntCells<ACC>) {
            // smallest of the nine products (weights are >= 0; the centre cell holds the largest)
            if (HAS_MASS && m == 0.0f)
                return;  // (a mass above MAX_M counts as 0: nine additions of +0)
            const float cmin = fminf(wx[0], wx[2]) * fminf(wy[0], wy[2]);
            // rare: a contribution that is not a multiple of the tile's quantum.  With per-particle masses also a NaN
            // (mass NaN or negative: every weight is NaN), which must not reach rn_scaled_u64: slow_record hands it to
            // the float atomic, and the map's pixel becomes NaN as in the reference
            if (HAS_MASS ? !(cmin >= Q.cmin) : cmin < Q.cmin) {
                const unsigned k = atomicAdd(s_nslow, 1u);
                if (k < kSlowCap)
                    s_slow[k] = make_uint2(c, i);
                else
                    slow_record<ACC, POW2>(xs, ys, sq, P, Q, tile, gmap, x0, y0, W);
                return;
            }
        }
        lds_t *cell0 = tile + (gy - y0) * W + (gx - x0);  // cell (gx - 1, gy - 1)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const int py = gy + b - 1;
            if (CHECK && (py < 0 || py >= nn))
                continue;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int px = gx + a - 1;
                if (CHECK && (px < 0 || px >= nn))
                    continue;
                lds_add<ACC, HAS_MASS>(cell0 + b * W + a, wx[a] * wy[b], P, Q);
            }
        }
    }
}

// One-level sort (one run per pending chunk: L.base): deposit this work item's share of every pending chunk into the
// LDS tile, the whole workgroup walking chunk by chunk.  CHECK: see deposit_record.
struct NoBoundary {
    __device__ __forceinline__ void operator()(int, int) const {}
};

// boundary(c, c_next) is called when the walk leaves chunk c for chunk c_next (c_end at the very end), after the
// records of c_next's first round have been requested: the NGP path folds a finished sub-file there.
template <int MAS, int ACC, bool POW2, bool HAS_MASS, bool CHECK, typename Boundary = NoBoundary>
__device__ __forceinline__ void tile_accumulate_chunks(const PendingList &L, const PassParams &P,
                                                typename AccT<ACC>::lds *tile, unsigned bin, unsigned part,
                                                unsigned nparts, int x0, int y0, int W, unsigned *s_nslow,
                                                uint2 *s_slow, typename AccT<ACC>::type *gmap, const TileQuantum &Q,
                                                int c_begin, int c_end, Boundary &&boundary = Boundary())
{
    const int tid = threadIdx.x;
#ifndef SLICER_K4_U
#define SLICER_K4_U 2
#endif
    // records in flight per lane and round.  A chunk brings a tile of the headline case ~1600 records: with 2 x 1024
    // slots per round one round per chunk, no slot group that only loads clamped duplicates (A/B in one call, round 3:
    // 450-454 us with 2 against 467-472 with 4; clustered and 2048^2 (6400 records per chunk and tile): equal)
    constexpr int U = SLICER_K4_U;
    // (dealing the waves to the pending chunks, so that all runs stream in at once, measured 699 us against 665 us for
    // this chunk-by-chunk walk: the kernel is bound by the LDS atomic pipe, not by the loads)
    // This part's share of each chunk's run, [len*part/nparts, len*(part+1)/nparts): lane c of every wave fetches
    // chunk c's bounds, so the (<= 8) dependent loads cost one latency instead of one per chunk.
    unsigned my_start = 0, my_end = 0;
    {
        const int c = c_begin + (int)lane_id();
        if (c < c_end) {
            const unsigned run0 = L.base[c][bin], len = L.base[c][bin + 1] - run0;
            my_start = run0 + (unsigned)(((unsigned long long)len * part) / nparts);
            my_end = run0 + (unsigned)(((unsigned long long)len * (part + 1)) / nparts);
        }
    }
    auto bounds = [&](int c, unsigned &a, unsigned &b) {
        a = (unsigned)__builtin_amdgcn_readlane((int)my_start, c - c_begin);
        b = (unsigned)__builtin_amdgcn_readlane((int)my_end, c - c_begin);
    };
    // The walk over (chunk, round of U * kTileBlock records) pairs is software-pipelined: the records of the next
    // round -- of the next chunk, if this one is exhausted -- are requested before the current round is deposited.
    auto advance = [&](int &c, unsigned &i0, unsigned &end) {  // -> false when the walk is over
        i0 += U * kTileBlock;
        while (i0 >= end) {
            if (++c >= c_end)
                return false;
            bounds(c, i0, end);
        }
        return true;
    };
    auto fetch = [&](int c, unsigned i0, unsigned end, float2 (&r)[U], float (&mr)[U]) {
        const float2 *__restrict__ sxy = L.sxy[c];
#pragma unroll
        for (int u = 0; u < U; u++) {
            // clamped, unconditional loads: a load under a branch makes the compiler drain the memory queue
            // before each one (s_waitcnt vmcnt(0)), which serialises the U loads
            const unsigned i = i0 + u * kTileBlock + tid;
            const unsigned ic = i < end ? i : end - 1;
            if (HAS_MASS) {
                const Rec3 v = reinterpret_cast<const Rec3 *>(sxy)[ic];
                r[u] = make_float2(v.x, v.y);
                mr[u] = v.m;
            } else {
                r[u] = sxy[ic];
            }
        }
    };
    int c = c_begin - 1;
    unsigned i0 = 0, end = 0;
    bool live = advance(c, i0, end);
    float2 r[U], rn[U];
    float mr[U], mn[U];
    if (live)
        fetch(c, i0, end, r, mr);
    while (live) {
        int cn = c;
        unsigned in0 = i0, endn = end;
        const bool more = advance(cn, in0, endn);
        if (more)
            fetch(cn, in0, endn, rn, mn);
        const float mconst = L.mconst[c], smc = L.sm_const[c];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned i = i0 + u * kTileBlock + tid;
            if (i >= end)
                continue;
            deposit_record<MAS, ACC, POW2, HAS_MASS, CHECK>(r[u].x, r[u].y, HAS_MASS ? mr[u] : 0.0f, mconst, smc,
                                                            (unsigned)c, i, P, Q, tile, gmap, x0, y0, W, s_nslow, s_slow);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            r[u] = rn[u];
            if (HAS_MASS)
                mr[u] = mn[u];
        }
        if (!more || cn != c)
            boundary(c, more ? cn : c_end);
        c = cn;
        i0 = in0;
        end = endn;
        live = more;
    }
}

// The records of one work item: a table of runs in LDS.  A run is a contiguous range of one pending chunk's sorted
// records: the chunk's whole (plane, tile) range with the one-level sort (k_bin_scatter: one run per chunk), or the
// tile's range inside one item of the two-level sort (k_sort2: one run per chunk and group, ~100 records each).  A part
// of a split bin takes the same fraction of every run.  The runs are walked as ONE sequence of records (s_pre: where
// each run starts in it), 64 consecutive records per wave instruction whatever the run lengths are.
struct RunRef {
    unsigned chunk, start;  // records [start, start + length) of L.sxy[chunk]; length = s_pre[k + 1] - s_pre[k]
};
constexpr int kMaxRuns = kMaxPendingRuns * kMaxSortGroups;
constexpr unsigned kWalkWindow = 65536;  // records walked per s_first table (kWalkWindow / 64 entries)

struct RunTable {
    RunRef *run;            // [kMaxRuns]
    unsigned *pre;          // [kMaxRuns + 1] exclusive prefix of the run lengths
    unsigned short *first;  // [kWalkWindow / 64] run that holds record 64 c of the current window
    const float2 **sxy;     // [kMaxPending] sorted records of every pending chunk
    float2 *mc;             // [kMaxPending] {mconst, sqrtf(mconst)} of every pending chunk
    int n;
};
constexpr size_t kRunTableBytes = sizeof(RunRef) * kMaxRuns + 4 * (kMaxRuns + 1) + 4 + 2 * (kWalkWindow / 64) +
                                  16 * kMaxPending;

__device__ __forceinline__ RunTable run_table_at(unsigned char *p)  // p: 8-byte aligned
{
    RunTable R;
    R.sxy = reinterpret_cast<const float2 **>(p);
    R.mc = reinterpret_cast<float2 *>(p + 8 * kMaxPending);
    R.run = reinterpret_cast<RunRef *>(p + 16 * kMaxPending);
    R.pre = reinterpret_cast<unsigned *>(R.run + kMaxRuns);
    R.first = reinterpret_cast<unsigned short *>(R.pre + kMaxRuns + 2);
    R.n = 0;
    return R;
}

// Fill the run table of (bin, part); every thread of the workgroup calls it (it holds barriers).
__device__ __forceinline__ void build_run_table(const PendingList &L, const BinGeom &G, unsigned bin, unsigned part,
                                                unsigned nparts, RunTable &R)
{
    const int tid = threadIdx.x;
    const int n_runs = L.run0[L.n];
    R.n = n_runs;
    if (tid < L.n) {
        R.sxy[tid] = L.sxy[tid];
        R.mc[tid] = make_float2(L.mconst[tid], L.sm_const[tid]);
    }
    for (int k = tid; k < n_runs; k += kTileBlock) {
        int c = 0;
        while (c + 1 < L.n && k >= L.run0[c + 1])
            c++;
        unsigned a, e;
        if (L.ptab[c]) {  // two-level sort: item (unit, group) of chunk c, entry tile-in-unit
            const unsigned unit = bin / (unsigned)G.tiles_per_unit, t = bin % (unsigned)G.tiles_per_unit;
            const unsigned g = (unsigned)(k - L.run0[c]);
            const unsigned *tab = L.ptab[c] + ((size_t)unit * (size_t)L.ngroups[c] + g) * (size_t)(G.tiles_per_unit + 1);
            a = tab[t];
            e = tab[t + 1];
        } else {
            a = L.base[c][bin];
            e = L.base[c][bin + 1];
        }
        const unsigned len = e - a;
        const unsigned lo = (unsigned)(((unsigned long long)len * part) / nparts);
        const unsigned hi = (unsigned)(((unsigned long long)len * (part + 1)) / nparts);
        RunRef r;
        r.chunk = (unsigned)c;
        r.start = a + lo;
        R.run[k] = r;
        R.pre[k + 1] = hi - lo;  // (lengths first; the prefix follows)
    }
    __syncthreads();
    if (tid < 64) {  // exclusive prefix over <= 256 lengths: four per lane of wave 0
        constexpr int PER = kMaxRuns / 64;
        unsigned v[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int k = tid * PER + j;
            v[j] = k < n_runs ? R.pre[k + 1] : 0u;
            sum += v[j];
        }
        unsigned x = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)x, d);
            if (tid >= d)
                x += y;
        }
        unsigned e = x - sum;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int k = tid * PER + j;
            e += v[j];
            if (k < n_runs)
                R.pre[k + 1] = e;
        }
        if (tid == 0)
            R.pre[0] = 0;
    }
    __syncthreads();
}

// Deposit the runs [k_begin, k_end) of the table into the LDS tile.  Every thread of the workgroup calls it (barriers
// around the s_first table); inside, every WAVE walks on its own: the records of the runs form one sequence, cut into
// pieces of 64; wave w takes pieces w, w + 16, ... -- two in flight, the next two requested before the current ones are
// deposited.  A lane finds its record's run from the piece's first run (s_first) and the run boundaries that follow.
// CHECK: see deposit_record.
template <int MAS, int ACC, bool POW2, bool HAS_MASS, bool CHECK>
__device__ __forceinline__ void tile_accumulate(const PassParams &P, typename AccT<ACC>::lds *tile, const RunTable &R,
                                                int k_begin, int k_end, int x0, int y0, int W, unsigned *s_nslow,
                                                uint2 *s_slow, typename AccT<ACC>::type *gmap, const TileQuantum &Q)
{
    const unsigned lane = lane_id();
    const int wave = threadIdx.x >> 6;
    constexpr int NW = kTileBlock / 64;
#ifndef SLICER_K4_UR
#define SLICER_K4_UR 2
#endif
    constexpr int U = SLICER_K4_UR;  // pieces (of 64 records) in flight per wave
    const unsigned q_begin = R.pre[k_begin], q_end = R.pre[k_end];
    for (unsigned w0 = q_begin; w0 < q_end; w0 += kWalkWindow) {  // (one window unless a tile holds > 65536 records)
        const unsigned w1 = q_end - w0 > kWalkWindow ? w0 + kWalkWindow : q_end;
        const unsigned npiece = (w1 - w0 + 63) >> 6;
        if (w0 != q_begin)
            __syncthreads();  // the previous window's table is no longer read
        for (unsigned pc = threadIdx.x; pc < npiece; pc += kTileBlock) {  // run that holds the piece's first record
            const unsigned q = w0 + (pc << 6);
            int lo = k_begin, hi = k_end - 1;  // largest k with pre[k] <= q
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (R.pre[mid] <= q)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            R.first[pc] = (unsigned short)lo;
        }
        __syncthreads();
        struct Rec {
            float2 r;
            float m;
            unsigned i, c;  // record index inside its chunk, chunk (c = ~0: no record)
        };
        auto fetch = [&](unsigned pc, Rec &o) {
            o.c = 0xFFFFFFFFu;
            o.i = 0;
            o.r = make_float2(0.f, 0.f);
            o.m = 0.f;
            if (pc >= npiece)
                return;
            const unsigned q = w0 + (pc << 6) + lane;
            const unsigned qc = q < w1 ? q : w1 - 1;  // clamped: an unconditional load (a load under a lane-dependent
                                                        // branch makes the compiler drain the memory queue first)
            int k = R.first[pc];
            while (qc >= R.pre[k + 1])
                k++;
            const RunRef rr = R.run[k];
            const unsigned i = rr.start + (qc - R.pre[k]);
            const float2 *__restrict__ sxy = R.sxy[rr.chunk];
            if (HAS_MASS) {
                const Rec3 v = reinterpret_cast<const Rec3 *>(sxy)[i];
                o.r = make_float2(v.x, v.y);
                o.m = v.m;
            } else {
                o.r = sxy[i];
            }
            o.i = i;
            o.c = q < w1 ? rr.chunk : 0xFFFFFFFFu;
        };
        Rec cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            fetch((unsigned)wave + (unsigned)(u * NW), cur[u]);
        for (unsigned pc = (unsigned)wave; pc < npiece; pc += U * NW) {
#pragma unroll
            for (int u = 0; u < U; u++)
                fetch(pc + (unsigned)((U + u) * NW), nxt[u]);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const unsigned c = cur[u].c, i = cur[u].i;
                if (c == 0xFFFFFFFFu)
                    continue;
                const float2 mc = R.mc[c];
                deposit_record<MAS, ACC, POW2, HAS_MASS, CHECK>(cur[u].r.x, cur[u].r.y, cur[u].m, mc.x, mc.y, c, i, P, Q,
                                                                tile, gmap, x0, y0, W, s_nslow, s_slow);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                cur[u] = nxt[u];
        }
    }
}

// the k-fold sequential f32 sum s <- fl(s + m) of utilities.cpp:75: what a pixel of the reference's per-file NGP map holds
__device__ __forceinline__ float ngp_seq_sum(unsigned k, float m)
{
    float s = 0.0f;
    for (unsigned j = 0; j < k; j++)
        s = s + m;
    return s;
}

// ---- heavy bins: wave-level pre-reduction before the LDS atomic ---------------------------------------------------
// A bin that k_build_items split into parts holds a halo core: many records in a few pixels.  64 lanes adding to the
// same LDS cell serialise (the 9 ds_add of a wave cost ~64x their usual LDS time), so the parts of such bins first ask
// whether every active lane of the wave targets the same cell; if so the nine contributions are summed across the wave
// (xor butterfly) and one lane issues the nine atomics.  Sums are reordered (allowed in the F32 / F64 modes, exact in
// FIXED64: integers); waves that straddle several cells fall back to per-lane atomics.
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += (unsigned long long)__shfl_xor((long long)v, off);
    return v;
}

// One run of a heavy bin: the records [start, end) of one pending chunk's sorted records sxy, {mconst, sm_const} the
// chunk's constant mass and its root.  (The NGP count kernels never come here: their branch of the kernel walks even
// the parts of a split bin with the plain loop.)
template <int MAS, int ACC, bool POW2, bool HAS_MASS>
__device__ __forceinline__ void merged_run(const float2 *__restrict__ sxy, float mconst, float sm_const, unsigned start,
                                           unsigned end, const PassParams &P, typename AccT<ACC>::lds *tile, int x0,
                                           int y0, int W, typename AccT<ACC>::type *gmap, const TileQuantum &Q)
{
    static_assert(ACC != kCountU32, "the NGP count kernels have no heavy-bin walk");
    const int tid = threadIdx.x;
    const int nn = P.nn;
    // every lane of a wave runs every iteration of its wave (no divergent exit: the butterfly needs all lanes)
    for (unsigned i0 = start; i0 < end; i0 += kTileBlock) {
        const unsigned i = i0 + tid;
        const bool act = i < end;
        float2 r = make_float2(0.f, 0.f);
        float m = mconst, sq = sm_const;
        if (HAS_MASS) {
            Rec3 v{0.f, 0.f, 0.f};
            if (act)
                v = reinterpret_cast<const Rec3 *>(sxy)[i];
            r = make_float2(v.x, v.y);
            m = cap_mass(v.m);
            sq = sqrt_mass(m);
        } else if (act) {
            r = sxy[i];
        }
        const int gx = grid_index<POW2>(r.x, P), gy = grid_index<POW2>(r.y, P);
        const int cell = act ? (gy - y0) * W + (gx - x0) : -1;  // cell (gx - 1, gy - 1) of the halo'd tile
        const unsigned long long am = __ballot(act);
        if (am == 0ull)
            continue;
        const int lead = (int)__builtin_ctzll(am);
        const int cell0 = __shfl(cell, lead);
        const bool uniform = __ballot(act && cell != cell0) == 0ull;
        if (MAS == kNGP) {
            if (uniform) {
                const double tot = wave_sum(act ? (double)m : 0.0);
                if ((int)lane_id() == lead)
                    atomicAdd(reinterpret_cast<double *>(tile + cell0 + W + 1), tot);
            } else if (act) {
                atomicAdd(reinterpret_cast<double *>(tile + cell + W + 1), (double)m);
            }
            continue;
        }
        float wx[3], wy[3];
        tsc_axis<POW2>(r.x, gx, P, wx);
        tsc_axis<POW2>(r.y, gy, P, wy);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            wx[a] = sq * wx[a];
            wy[a] = sq * wy[a];
        }
#pragma unroll
        for (int b = 0; b < 3; b++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                // map-edge tests as in the CHECK variant (heavy border tiles are rare enough not to specialise)
                const int px = gx + a - 1, py = gy + b - 1;
                bool in = act && px >= 0 && px < nn && py >= 0 && py < nn;
                const float cf = wx[a] * wy[b];
                if (kIntCells<ACC>) {  // contributions that are no multiple of the tile's quantum bypass the tile
                    const double t = (double)cf * Q.scale;
                    if (in && t != rint(t)) {
                        atomicAdd(gmap + (size_t)px + (size_t)nn * (size_t)py, (typename AccT<ACC>::type)cf);
                        in = false;
                    }
                }
                if (uniform) {  // wave-uniform branch
                    if (kIntCells<ACC>) {
                        const unsigned long long tot = wave_sum(in ? rn_scaled_u64(cf, Q.scale) : 0ull);
                        if ((int)lane_id() == lead && tot)
                            atomicAdd(reinterpret_cast<unsigned long long *>(tile + cell0 + b * W + a), tot);
                    } else if (ACC == kFixed64) {
                        const bool add = in && (!HAS_MASS || contribution_finite(cf));  // (see lds_add)
                        const unsigned long long tot = wave_sum(add ? rn_scaled_u64(cf, P.fixed_scale) : 0ull);
                        if ((int)lane_id() == lead && tot)
                            atomicAdd(reinterpret_cast<unsigned long long *>(tile + cell0 + b * W + a), tot);
                    } else {
                        const double tot = wave_sum(in ? (double)cf : 0.0);
                        if ((int)lane_id() == lead && tot != 0.0)
                            atomicAdd(reinterpret_cast<double *>(tile + cell0 + b * W + a), tot);
                    }
                } else if (in) {
                    lds_add<ACC, HAS_MASS>(tile + cell + b * W + a, cf, P, Q);
                }
            }
        }
    }
}

// The heavy-bin walk of the one-level sort: this part's share of every pending chunk's run, the whole workgroup on one
// chunk at a time.
template <int MAS, int ACC, bool POW2, bool HAS_MASS>
__device__ __forceinline__ void tile_accumulate_merged_chunks(const PendingList &L, const PassParams &P,
                                                       typename AccT<ACC>::lds *tile, unsigned bin, unsigned part,
                                                       unsigned nparts, int x0, int y0, int W,
                                                       typename AccT<ACC>::type *gmap, const TileQuantum &Q)
{
    for (int c = 0; c < L.n; c++) {
        const unsigned run0 = L.base[c][bin], len = L.base[c][bin + 1] - run0;
        const unsigned start = run0 + (unsigned)(((unsigned long long)len * part) / nparts);
        const unsigned end = run0 + (unsigned)(((unsigned long long)len * (part + 1)) / nparts);
        merged_run<MAS, ACC, POW2, HAS_MASS>(L.sxy[c], L.mconst[c], L.sm_const[c], start, end, P, tile, x0, y0, W, gmap, Q);
    }
}

// ... and of the two-level sort: the runs of the table, one after the other.
template <int MAS, int ACC, bool POW2, bool HAS_MASS>
__device__ __forceinline__ void tile_accumulate_merged(const PendingList &L, const PassParams &P,
                                                       typename AccT<ACC>::lds *tile, const RunTable &R, int x0, int y0,
                                                       int W, typename AccT<ACC>::type *gmap, const TileQuantum &Q)
{
    for (int kk = 0; kk < R.n; kk++) {
        const RunRef rr = R.run[kk];
        const int c = __builtin_amdgcn_readfirstlane((int)rr.chunk);
        const unsigned start = (unsigned)__builtin_amdgcn_readfirstlane((int)rr.start);
        const unsigned end = start + (unsigned)__builtin_amdgcn_readfirstlane((int)(R.pre[kk + 1] - R.pre[kk]));
        merged_run<MAS, ACC, POW2, HAS_MASS>(L.sxy[c], L.mconst[c], L.sm_const[c], start, end, P, tile, x0, y0, W, gmap, Q);
    }
}

// Visit every cell of a W x H LDS tile (W = 64 k + 2): a wave per row with its lanes along the row for the first W - 2
// columns, then the two halo columns on the right as one dense range -- no division by the run-time row length and no
// nearly empty trip for the two cells beyond a multiple of 64.
template <typename Fn>
__device__ __forceinline__ void for_each_tile_cell(int W, int H, Fn &&fn)
{
    const int tid = threadIdx.x;
    for (int row = tid >> 6; row < H; row += kTileBlock / 64)
        for (int col = tid & 63; col < W - 2; col += 64)
            fn(row, col);
    for (int i = tid; i < 2 * H; i += kTileBlock)
        fn(i >> 1, W - 2 + (i & 1));
}

// RUNS: the pending chunks come from the two-level sort (a table of runs per tile, walked wave by wave); otherwise one
// run per chunk (L.base), walked by the whole workgroup.
// Registers: the TSC variants need ~54 and run two workgroups per CU.  The NGP count kernel keeps 16 pixel values per
// lane in registers for its in-tile fold; without the species' own map (HAS_MASS slot = false) it is held to 64 registers
// (28 bytes of scratch, touched at the file boundaries only) for the second workgroup per CU: tile kernel 615 -> 490 us,
// --mas ngp 2.05 -> 1.92 ms per snapshot (A/B in one call, profiles/r03_k4_stage_costs.log).  With the second map (16
// more values) the same limit spills 120 bytes and doubles the kernel's time (755 -> 1470 us): that variant stays at
// one workgroup per CU.
#ifndef SLICER_K4_NGP_WAVES
#define SLICER_K4_NGP_WAVES 8
#endif
template <int MAS, int ACC, bool POW2, bool HAS_MASS, bool RUNS>
__global__ __launch_bounds__(kTileBlock, (MAS == kNGP && ACC == kCountU32 && !HAS_MASS) ? SLICER_K4_NGP_WAVES : 4) void
k_tile_deposit(PendingList L, PassParams P, BinGeom G, Targets T, TileItems I, NgpFold F)
{
    using acc_t = typename AccT<ACC>::type;
    using lds_t = typename AccT<ACC>::lds;
    // 16-byte aligned by declaration: ds_add_u64 / ds_add_f64 on a cell that is only 4-byte aligned FAULTS (round 2: a
    // static __shared__ array in front of an unaligned dynamic array did exactly that).  The attribute makes the
    // compiler pad whatever static LDS precedes the dynamic segment; the small tables of this kernel live behind the tile.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    lds_t *tile = reinterpret_cast<lds_t *>(smem_raw);
    static_assert(alignof(lds_t) <= 16 && sizeof(lds_t) <= 8, "tile cells are 4- or 8-byte scalars");

    unsigned bin = blockIdx.x, part = 0;
    if (blockIdx.x >= (unsigned)G.nbins) {
        const unsigned j = blockIdx.x - (unsigned)G.nbins;
        if (j >= *I.n_extra)
            return;
        const uint2 item = I.extra[j];
        bin = item.x, part = item.y;
    }
    const unsigned nparts = I.nparts[bin];
    if (nparts == 0)
        return;
    const int unit = bin / G.tiles_per_unit;
    const int t = bin % G.tiles_per_unit;
    const int plane = unit / G.units_per_plane;
    const int band = unit % G.units_per_plane;
    const int x0 = (t % G.ntx) << G.tw_log2;
    const int y0 = (band * G.rows_per_unit + t / G.ntx) << G.th_log2;
    const int W = (1 << G.tw_log2) + 2, H = (1 << G.th_log2) + 2;
    const int cells = W * H;
    const int tid = threadIdx.x;
    const int nn = P.nn;

    // behind the tile (no static __shared__ in this kernel: it would sit in front of the dynamic array and leave the
    // 8-byte cells 4-byte aligned -- misaligned 64-bit LDS atomics fault): a counter, then the list of noted records
    unsigned char *behind = smem_raw + ((sizeof(lds_t) * (size_t)cells + 7) & ~(size_t)7);
    unsigned &s_nslow = *reinterpret_cast<unsigned *>(behind);
    uint2 *s_slow = reinterpret_cast<uint2 *>(behind) + 1;  // [kSlowCap] {chunk, record}: integer-cell modes only
    RunTable R = run_table_at(behind + 8 + (kIntCells<ACC> ? kSlowCap * sizeof(uint2) : 0));
    acc_t *gmap = reinterpret_cast<acc_t *>(T.acc[plane]);
    TileQuantum Q{P.tile_scale, P.tile_inv_scale, P.tile_cmin};
    if (kIntCells<ACC> && HAS_MASS) {
        // per-particle masses: the scale follows the largest selected mass of the species (bits of a non-negative f32)
        const unsigned mm = *T.max_mass;
        const int le = mm ? (int)((mm >> 23) & 0xFFu) - 126 : 0;  // 2^le > m for every m <= that maximum
        Q.scale = __builtin_ldexp(1.0, 49 - le);
        Q.inv_scale = __builtin_ldexp(1.0, le - 49);
        Q.cmin = __builtin_ldexpf(1.0f, le - 25);
    }
    for (int i = tid; i < cells; i += kTileBlock)
        tile[i] = (lds_t)0;
    if (tid == 0)
        s_nslow = 0;
    if (RUNS)
        build_run_table(L, G, bin, part, nparts, R);  // (ends in a barrier: tile zeroed, table complete)
    else
        __syncthreads();

    // the halo [x0 - 1, x0 + W - 2] x [y0 - 1, y0 + H - 2] inside the map: no cell of this tile needs the edge test
    const bool interior = x0 >= 1 && y0 >= 1 && x0 + W - 2 < nn && y0 + H - 2 < nn;
    if constexpr (MAS == kNGP && ACC == kCountU32) {
        // NGP counts: one sub-file after the other (chunks of a file are neighbours in the list).  A file marked `fold`
        // is folded into the f32 maps right here -- this workgroup is the only one that touches these pixels in this
        // launch (NGP records hit cells of their own tile only, and no tile is split when F.on), so the pixel values
        // travel in registers from the first file to the last: lane `tid` owns the tile's cells tid, tid + 1024, ...
        // Any other file's counts go to the global count map.
        constexpr int CPT = 16;  // 128 x 128 cells / 1024 lanes
        // (the NGP-count instantiations have no per-particle masses; their HAS_MASS flag says instead whether the
        // species' own map is kept next to the all-types map: 16 more registers per lane, one workgroup per CU less)
        constexpr bool TYPE_MAP = HAS_MASS;
        float rt[CPT], ri[CPT];
        float *tot = F.tot[plane], *toti = F.toti[plane];
        const int tw = 1 << G.tw_log2, ncell = tw << G.th_log2;
        // lane's j-th cell: tile cell i = j * 1024 + tid, i.e. LDS cell cell0 + j * cstride, pixel idx0 + j * pstride
        const int row0 = tid >> G.tw_log2, col0 = tid & (tw - 1);
        const int rows_per_j = kTileBlock >> G.tw_log2;  // (tile widths are <= 1024)
        const int cell0 = (row0 + 1) * W + col0 + 1, cstride = rows_per_j * W;
        const size_t idx0 = (size_t)(x0 + col0) + (size_t)nn * (size_t)(y0 + row0), pstride = (size_t)nn * (size_t)rows_per_j;
        unsigned inmask = 0;  // bit j: that cell exists and lies inside the map
#pragma unroll
        for (int j = 0; j < CPT; j++)
            if (j * kTileBlock + tid < ncell && x0 + col0 < nn && y0 + row0 + j * rows_per_j < nn)
                inmask |= 1u << j;
        if (F.on) {
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                const bool in = inmask >> j & 1u;
                rt[j] = in ? tot[idx0 + j * pstride] : 0.0f;
                ri[j] = (TYPE_MAP && in && toti) ? toti[idx0 + j * pstride] : 0.0f;
            }
        }
        unsigned touched = 0;
        // one sub-file after the other: the runs of its chunks are deposited (every wave walks its share), then the
        // file's counts are folded, or flushed to the count map
        auto boundary = [&](int c) {
            __syncthreads();
            if (F.on && L.fold[c]) {
                const float m = L.mconst[c];
                unsigned kk[CPT];
#pragma unroll
                for (int j = 0; j < CPT; j++)  // (all LDS reads first: one latency)
                    kk[j] = (inmask >> j & 1u) ? (unsigned)tile[cell0 + j * cstride] : 0u;
#pragma unroll
                for (int j = 0; j < CPT; j++) {
                    if (kk[j] == 0)
                        continue;
                    tile[cell0 + j * cstride] = (lds_t)0;
                    const float v = ngp_seq_sum(kk[j], m);
                    rt[j] = rt[j] + v;  // tot += mapxyi, toti += mapxyi   densitymaps.cpp:511-513
                    if (TYPE_MAP)
                        ri[j] = ri[j] + v;
                    touched |= 1u << j;
                }
            } else {
                auto flush = [&](int row, int col) {
                    const unsigned k = (unsigned)tile[row * W + col];
                    if (k == 0)
                        return;
                    tile[row * W + col] = (lds_t)0;
                    atomicAdd(gmap + (size_t)(x0 - 1 + col) + (size_t)nn * (size_t)(y0 - 1 + row), (acc_t)k);
                };
                for_each_tile_cell(W, H, flush);
            }
            __syncthreads();
        };
        if (RUNS) {
            for (int c0 = 0; c0 < L.n;) {
                int c1 = c0 + 1;
                while (c1 < L.n && L.file_id[c1] == L.file_id[c0])
                    c1++;
                tile_accumulate<MAS, ACC, POW2, false, false>(P, tile, R, L.run0[c0], L.run0[c1], x0, y0, W, &s_nslow,
                                                              s_slow, gmap, Q);
                boundary(c0);
                c0 = c1;
            }
        } else {
            // one walk over all pending chunks; when it leaves the last chunk of a sub-file (the next round's records
            // are already on their way) the file's counts are folded, or flushed to the count map
            auto leave = [&](int c, int c_next) {
                if (c_next < L.n && L.file_id[c_next] == L.file_id[c])
                    return;
                boundary(c);
            };
            tile_accumulate_chunks<MAS, ACC, POW2, false, false>(L, P, tile, bin, part, nparts, x0, y0, W, &s_nslow, s_slow,
                                                                 gmap, Q, 0, L.n, leave);
        }
#pragma unroll
        for (int j = 0; j < CPT; j++)
            if (touched >> j & 1u) {
                tot[idx0 + j * pstride] = rt[j];
                if (TYPE_MAP && toti)
                    toti[idx0 + j * pstride] = ri[j];
            }
    } else {
        // pre-reduction only for bins far beyond a tile's usual load (>= 8 parts = 131072 records: a halo core); a bin
        // that is merely split in two or three is faster through the plain loop (--clustered: 810 us with, 700 us
        // without)
        if (RUNS) {
            if (nparts >= kMergeParts)
                tile_accumulate_merged<MAS, ACC, POW2, HAS_MASS>(L, P, tile, R, x0, y0, W, gmap, Q);
            else if (MAS == kNGP || interior)
                tile_accumulate<MAS, ACC, POW2, HAS_MASS, false>(P, tile, R, 0, R.n, x0, y0, W, &s_nslow, s_slow, gmap, Q);
            else
                tile_accumulate<MAS, ACC, POW2, HAS_MASS, true>(P, tile, R, 0, R.n, x0, y0, W, &s_nslow, s_slow, gmap, Q);
        } else {
            if (nparts >= kMergeParts)
                tile_accumulate_merged_chunks<MAS, ACC, POW2, HAS_MASS>(L, P, tile, bin, part, nparts, x0, y0, W, gmap, Q);
            else if (MAS == kNGP || interior)
                tile_accumulate_chunks<MAS, ACC, POW2, HAS_MASS, false>(L, P, tile, bin, part, nparts, x0, y0, W, &s_nslow,
                                                                        s_slow, gmap, Q, 0, L.n);
            else
                tile_accumulate_chunks<MAS, ACC, POW2, HAS_MASS, true>(L, P, tile, bin, part, nparts, x0, y0, W, &s_nslow,
                                                                       s_slow, gmap, Q, 0, L.n);
        }
        __syncthreads();
        if (kIntCells<ACC>) {
            // the records noted in the loop: those of their contributions that are exact multiples of the quantum go
            // into the tile like all others, the vanishing ones straight to the global map
            const unsigned ns = s_nslow < kSlowCap ? s_nslow : kSlowCap;
            for (unsigned e = tid; e < ns; e += kTileBlock) {
                const uint2 w = s_slow[e];
                if (HAS_MASS) {
                    const Rec3 r = reinterpret_cast<const Rec3 *>(L.sxy[w.x])[w.y];
                    slow_record<ACC, POW2>(r.x, r.y, sqrt_mass(cap_mass(r.m)), P, Q, tile, gmap, x0, y0, W);
                } else {
                    const float2 r = L.sxy[w.x][w.y];
                    slow_record<ACC, POW2>(r.x, r.y, L.sm_const[w.x], P, Q, tile, gmap, x0, y0, W);
                }
            }
            __syncthreads();
        }

        // flush: consecutive lanes -> consecutive pixels of one map row (shaped atomics).  (Round 3 measured the
        // alternative for the cells only this workgroup adds to -- plain load + add + store, stores running at ~6 TB/s
        // against ~1.3 TB/s of added bytes for memory-side float atomics: tile kernel 471 -> 873 us.  The atomics are
        // fire-and-forget, the read-modify-write puts an HBM round trip per cell row on the flushing wave.)
        auto flush = [&](int row, int col) {
            const lds_t v = tile[row * W + col];
            const int px = x0 - 1 + col, py = y0 - 1 + row;
            if (v == (lds_t)0 || px < 0 || px >= nn || py < 0 || py >= nn)
                return;
            acc_t *cell = gmap + (size_t)px + (size_t)nn * (size_t)py;
            if (kIntCells<ACC>)  // exact tile sum -> one rounding to the accumulator type
                atomicAdd(cell, (acc_t)((double)v * Q.inv_scale));
            else
                atomicAdd(cell, (acc_t)v);
        };
        for_each_tile_cell(W, H, flush);
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
size_t tile_lds_bytes(const BinGeom &G, int acc, bool runs)
{
    const size_t elem = acc == kCountU32 ? 4 : 8;
    const size_t cells = (size_t)((1 << G.tw_log2) + 2) * (size_t)((1 << G.th_log2) + 2);
    return ((elem * cells + 7) & ~(size_t)7) + 8 + ((acc == kF32I || acc == kF64I) ? kSlowCap * sizeof(uint2) : 0) +
           (runs ? kRunTableBytes : 0);  // (the run table of the two-level sort's walk)
}

template <int MAS, int ACC>
static hipError_t launch_k4(bool pow2, bool has_mass, const PassParams &P, const BinGeom &G, const PendingList &L,
                            const Targets &T, const TileItems &I, const NgpFold &F, unsigned max_items, hipStream_t s)
{
    using True = std::true_type;
    using False = std::false_type;
    const bool runs = L.tot != nullptr;
    const size_t lds = tile_lds_bytes(G, ACC, runs);
    auto kernel = [](auto p2, auto hm, auto rn) -> decltype(&k_tile_deposit<MAS, ACC, false, false, false>) {
        // binned_chunk (binned_pass.cpp) turns the two-level sort on, and with it L.tot, only without per-particle masses
        if constexpr (hm() && rn() && !(MAS == kNGP && ACC == kCountU32))  // (count kernels: the flag is the type map)
            return nullptr;
        else
            return k_tile_deposit<MAS, ACC, p2(), hm(), rn()>;
    };
    auto by_runs = [&](auto p2, auto hm) { return runs ? kernel(p2, hm, True{}) : kernel(p2, hm, False{}); };
    auto by_mass = [&](auto p2) { return has_mass ? by_runs(p2, True{}) : by_runs(p2, False{}); };
    const auto kern = pow2 ? by_mass(True{}) : by_mass(False{});
    if (!kern)
        return hipErrorInvalidValue;
    return launch_with_lds(kern, max_items, kTileBlock, lds, /*raise_above=*/48 * 1024, s, L, P, G, T, I, F);
}

size_t tile_items_bytes(const BinGeom &G, uint64_t total_particles)
{
    const uint64_t max_extra = total_particles / kItemRecs + 1;
    return 16 + (size_t)(G.nbins + (G.nbins & 1)) * 4 + max_extra * sizeof(uint2);  // counters | nparts | extra
}

hipError_t launch_tile_deposit(const LaunchCfg &cfg, const PassParams &P, const BinGeom &G, const PendingList &L,
                               const Targets &T, const NgpFold &F, void *items_ws, unsigned epoch,
                               uint64_t total_particles, int int_mode, bool *int_cells_used, hipStream_t s)
{
    *int_cells_used = false;
    // total_particles bounds the number of records (each particle emits at most one on this path).  Workspace:
    // two counters (used alternately: launch `epoch` reads [epoch & 1] and zeroes the other one) | nparts | extra
    const unsigned max_items = (unsigned)((uint64_t)G.nbins + total_particles / kItemRecs + 1);
    TileItems I;
    unsigned *counters = reinterpret_cast<unsigned *>(items_ws);
    I.n_extra = counters + (epoch & 1u);
    I.next_n_extra = counters + ((epoch + 1u) & 1u);
    I.nparts = counters + 4;
    I.extra = reinterpret_cast<uint2 *>(I.nparts + G.nbins + (G.nbins & 1));
    const bool pow2 = P.pow2 != 0;
    // TSC in the F32 / F64 modes: integer tile cells (int_mode, the handle's option k4_int: 0 keeps the
    // f64 cells, 2 forces the integer ones).  They pay where the records dominate (2048^2 x 4 planes, 65536 particles per bin: 370 against 622 us);
    // a launch with few records per tile is mostly tile zeroing and flushing, where the u64 -> float conversion of every
    // cell costs what the cheaper LDS atomic saves (8192^2 x 4 planes, 4096 per bin: 1242 against 1205 us; 2048 per bin:
    // equal) -- below 2048 particles per bin the f64 cells stay.
    // Decided before the work items are built: the cells of the launch set how many records a bin may hold and stay
    // whole (kWholeRecsInt).  The bound on the extra items (max_items, tile_items_bytes: total_particles / kItemRecs + 1)
    // holds with either cap, since a bin of t records adds ceil(t / kItemRecs) - 1 <= t / kItemRecs items.
    bool int_launch = false;
    if (cfg.mas != kNGP && (cfg.acc == kF32 || cfg.acc == kF64) &&
        (int_mode == 2 || (int_mode == 1 && total_particles / (uint64_t)G.nbins >= 2048))) {
        int_launch = cfg.has_mass;  // (per-particle masses: the quantum follows the largest mass the sort kernel saw)
        if (!cfg.has_mass) {        // one quantum per launch: all pending chunks carry the same constant mass
            int_launch = L.mconst[0] == P.mconst;
            for (int c = 1; c < L.n; c++)
                int_launch = int_launch && L.mconst[c] == L.mconst[0];
        }
    }
    k_build_items<<<(G.nbins + 255) / 256, 256, 0, s>>>(L, G.nbins, I, (cfg.mas == kNGP && cfg.acc == kCountU32 && F.on) ? 1 : 0,
                                                        int_launch ? kWholeRecsInt : kWholeRecs);
    if (cfg.mas == kNGP) {
        if (cfg.acc == kCountU32) {
            // (has_mass slot of the count kernels: keep the species' own map in the in-tile fold)
            return launch_k4<kNGP, kCountU32>(pow2, F.on && F.toti[0] != nullptr, P, G, L, T, I, F, max_items, s);
        }
        return launch_k4<kNGP, kF32>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
    }
    if (int_launch) {
        *int_cells_used = true;
        if (cfg.acc == kF32)
            return launch_k4<kTSC, kF32I>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
        return launch_k4<kTSC, kF64I>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
    }
    switch (cfg.acc) {
    case kF32: return launch_k4<kTSC, kF32>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
    case kF64: return launch_k4<kTSC, kF64>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
    case kFixed64: return launch_k4<kTSC, kFixed64>(pow2, cfg.has_mass, P, G, L, T, I, F, max_items, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace slicer
