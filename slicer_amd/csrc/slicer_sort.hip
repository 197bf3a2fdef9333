// slicer_sort.hip -- SLICER_ALGO_BINNED, K2 and K3: the scan over the per-workgroup histograms and the two sorts that
// move every record into its (plane, tile) bin's run (overview of the path: slicer_binned_common.hpp).
#include "slicer_binned_common.hpp"

#pragma clang fp contract(off)

namespace slicer {

// K1 (project + bin) lives in slicer_project_bin.hip.

// ---------------------------------------------------------------------------------------------
// K2a: per bin, exclusive prefix over workgroups + total: segment sums, a 32-way scan in LDS, prefix write.
// ---------------------------------------------------------------------------------------------
constexpr int kScanBins = 32;               // bins per workgroup of k_scan_blocks
constexpr int kScanSegs = 1024 / kScanBins;  // segments of the K1-workgroup axis

__global__ __launch_bounds__(1024) void k_scan_blocks(const unsigned short *__restrict__ hist16,
                                                      unsigned *__restrict__ prefix, unsigned *__restrict__ lex,
                                                      unsigned *__restrict__ gsum, int nblocks, int nbins)
{
    // 32 bins (a half-wave reads 64 contiguous bytes of a histogram row) x 32 segments of the workgroup axis:
    // 256 workgroups for 8192 bins, 16 rows per lane at 512 K1 workgroups.
    // Besides the per-(workgroup, bin) write cursors it leaves, for the bins of its group, the exclusive prefix of the
    // bin totals inside the group (lex) and the group's sum (gsum): the sort kernel turns those into bin bases itself
    // (a 256-entry scan per workgroup), which saves the single-workgroup scan launch that used to sit in between.
    __shared__ unsigned s_seg[kScanSegs][kScanBins];
    const int bl = threadIdx.x % kScanBins, seg = threadIdx.x / kScanBins;
    const int bin = blockIdx.x * kScanBins + bl;
    const size_t stride16 = (size_t)((nbins + 1) >> 1) * 2;
    const int per = (nblocks + kScanSegs - 1) / kScanSegs;
    const int lo = seg * per, hi = lo + per < nblocks ? lo + per : nblocks;
    // (up to kKeep rows per lane -- 512 K1 workgroups give 16 -- stay in registers between the two passes: one read)
    constexpr int kKeep = 16;
    unsigned short keep[kKeep];
    const bool kept = per <= kKeep;
    unsigned sum = 0;
    if (bin < nbins) {
        if (kept) {
#pragma unroll
            for (int j = 0; j < kKeep; j++) {
                keep[j] = lo + j < hi ? hist16[(size_t)(lo + j) * stride16 + bin] : (unsigned short)0;
                sum += keep[j];
            }
        } else {
            for (int b = lo; b < hi; b++)
                sum += hist16[(size_t)b * stride16 + bin];
        }
    }
    s_seg[seg][bl] = sum;
    __syncthreads();
    unsigned run = 0;
    for (int k = 0; k < seg; k++)
        run += s_seg[k][bl];
    if (bin < nbins) {
        if (kept) {
#pragma unroll
            for (int j = 0; j < kKeep; j++)
                if (lo + j < hi) {
                    prefix[(size_t)(lo + j) * nbins + bin] = run;
                    run += keep[j];
                }
        } else {
            for (int b = lo; b < hi; b++) {
                unsigned v = hist16[(size_t)b * stride16 + bin];
                prefix[(size_t)b * nbins + bin] = run;
                run += v;
            }
        }
    }
    if (seg == kScanSegs - 1) {  // lanes 992..1023: one half-wave holds the totals of the group's 32 bins
        const unsigned tot = bin < nbins ? run : 0u;
        unsigned x = tot;
#pragma unroll
        for (int d = 1; d < kScanBins; d <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)x, d, kScanBins);
            if (bl >= d)
                x += y;
        }
        if (bin < nbins)
            lex[bin] = x - tot;
        if (bl == kScanBins - 1)
            gsum[blockIdx.x] = x;
    }
}

// ---------------------------------------------------------------------------------------------
// K3: scatter records into their bin runs
// ---------------------------------------------------------------------------------------------
// One work item per (unit, K1 workgroup) pair (a unit is a plane, or a band of tile rows of a plane on large maps),
// taken by persistent 512-thread workgroups, two per CU.  An item's records are counting-sorted by tile in LDS
// (sub-batches of kSortBatch records, exchanged kSortStage at a time), so that the records of one (unit, tile) run
// are stored by adjacent lanes: a plain scatter issues one 32-byte sector write per 8-byte record (measured write
// amplification 4.2x), runs of 3-8 records cut that to 1-2 sectors per run.  The phases of an item (loads, scan,
// LDS exchange, stores) are serial inside a workgroup; the second workgroup of the CU fills the gaps (81 -> 70 us).
#ifndef SLICER_K3_BLOCK
#define SLICER_K3_BLOCK 512
#endif
constexpr int kSortBlock = SLICER_K3_BLOCK;
constexpr int kSortBatch = 8192;
#ifndef SLICER_K3_STAGE
#define SLICER_K3_STAGE 4096
#endif
#ifndef SLICER_K3_WAVES
#define SLICER_K3_WAVES 4  // waves per SIMD the register budget allows: two 512-thread workgroups per CU
#endif
constexpr int kSortStage = SLICER_K3_STAGE;  // sorted records staged in LDS at a time

__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *s_wave /*[kSortBlock/64]*/)
{
    // inclusive scan inside the wave, wave totals through LDS
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = (unsigned)__shfl_up((int)x, d);
        if ((int)lane_id() >= d)
            x += y;
    }
    const int w = threadIdx.x >> 6;
    if (lane_id() == 63)
        s_wave[w] = x;
    lds_barrier();
    unsigned off = 0;
    for (int k = 0; k < w; k++)
        off += s_wave[k];
    lds_barrier();
    return off + x - v;
}

template <bool HAS_MASS>
__global__ __launch_bounds__(kSortBlock, SLICER_K3_WAVES) void k_bin_scatter(const float2 *__restrict__ cxy,
                                                            const unsigned short *__restrict__ cbin,
                                                            const float *__restrict__ cm,
                                                            const unsigned *__restrict__ hist16w,
                                                            const unsigned *__restrict__ prefix,
                                                            const unsigned *__restrict__ lex,
                                                            const unsigned *__restrict__ gsum,
                                                            unsigned *__restrict__ base,
                                                            const unsigned *__restrict__ bcount, int nblocks,
                                                            BinGeom G, float2 *__restrict__ sxy,
                                                            float *__restrict__ sm, int count_planes, Targets T)
{
    extern __shared__ unsigned smem_sc[];
    const int tpp = G.tiles_per_unit;
    const int tw = (tpp + 1) >> 1;    // words of a packed u16 table
    unsigned *cnt = smem_sc;          // [tpp] u16 x2 per word: records of the sub-batch per tile (<= kSortBatch)
    unsigned *pos = cnt + tw;         // [tpp] u32 running sorted position of each tile (ends at start + cnt)
    unsigned *cur = pos + tpp;        // [tpp] u32 global write cursor of this unit minus the tile's sorted start
    float2 *sorted_xy = reinterpret_cast<float2 *>(cur + tpp + (tw & 1));
    unsigned short *sorted_tile = reinterpret_cast<unsigned short *>(sorted_xy + kSortStage);
    float *sorted_m = reinterpret_cast<float *>(sorted_tile + kSortStage);  // HAS_MASS only
    __shared__ unsigned s_wave[kSortBlock / 64];
    __shared__ unsigned s_gp[kMaxBins / kScanBins + 1];  // exclusive prefix of the scan kernel's group sums

    const int tid = threadIdx.x;
    // bin bases: base[bin] = s_gp[bin / 32] + lex[bin].  Every workgroup scans the (<= 1024) group sums for itself;
    // workgroup 0 also writes base[] out for the tile kernel and adds every plane's record count (= its selected
    // entries on the TSC path) to the counters.
    {
        const int ngroups = (G.nbins + kScanBins - 1) / kScanBins;
        constexpr int kPerLane = (kMaxBins / kScanBins + kSortBlock - 1) / kSortBlock;  // 2 at 512 threads
        unsigned v[kPerLane], sum = 0;
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int g = tid * kPerLane + j;
            v[j] = g < ngroups ? gsum[g] : 0u;
            sum += v[j];
        }
        unsigned e = block_exclusive_scan(sum, s_wave);
#pragma unroll
        for (int j = 0; j < kPerLane; j++) {
            const int g = tid * kPerLane + j;
            if (g < ngroups)
                s_gp[g] = e;
            e += v[j];
        }
        if (tid == kSortBlock - 1)
            s_gp[ngroups] = e;  // all records
        lds_barrier();
        if (blockIdx.x == 0) {
            for (int i = tid; i <= G.nbins; i += kSortBlock)
                base[i] = i < G.nbins ? s_gp[i / kScanBins] + lex[i] : s_gp[ngroups];
            if (tid < count_planes) {
                const int bpp = G.units_per_plane * G.tiles_per_unit;  // bins per plane
                auto at = [&](int i) { return i < G.nbins ? s_gp[i / kScanBins] + lex[i] : s_gp[ngroups]; };
                const unsigned c = at((tid + 1) * bpp) - at(tid * bpp);
                if (c)
                    atomicAdd(T.nsel[tid], (unsigned long long)c);
            }
        }
    }
    // Persistent workgroups: each takes the (unit, K1 workgroup) items b, b + gridDim.x, ...  item -> (unit, K1
    // workgroup) keeps an XCD's items on a contiguous range of K1 workgroups (gridDim.x is a multiple of 8, so
    // item & 7 is this workgroup's XCD): runs of one tile written by neighbouring K1 workgroups then meet in the
    // same L2.
    const int per_unit = 8 * ((nblocks + 7) / 8);
    const int per_xcd = per_unit / 8;
    const int per = (tpp + kSortBlock - 1) / kSortBlock;  // tiles per lane in the scan (<= 16: tiles_per_unit <= 8192)
    auto get16 = [](const unsigned *tab, unsigned t) { return (tab[t >> 1] >> ((t & 1u) * 16u)) & 0xFFFFu; };
    constexpr int R = kSortBatch / kSortBlock;  // records per lane and sub-batch
    // largest selected mass of the species (as the deposit sees it: above MAX_M counts as 0) -> the quantum of integer
    // tile cells (TileQuantum); masses are non-negative, so their bits order like the values.  One atomic per wave and
    // launch, and only if it can raise the maximum.
    float mass_max = 0.0f;
    for (int item = blockIdx.x; item < G.n_units * per_unit; item += gridDim.x) {
        const int plane = item / per_unit;  // the unit index (a whole plane unless the map is large)
        const int u = item % per_unit;
        const int lb = (u & 7) * per_xcd + (u >> 3);
        if (lb >= nblocks)
            continue;
        const unsigned count = bcount[(size_t)plane * nblocks + lb];
        if (count == 0)
            continue;
        lds_barrier();  // the previous item's tables are no longer read
        const unsigned *row = prefix + (size_t)lb * G.nbins + (size_t)plane * tpp;
        const unsigned *lrow = lex + (size_t)plane * tpp;
        const unsigned bin0 = (unsigned)plane * (unsigned)tpp;
        for (int i = tid; i < tpp; i += kSortBlock)
            cur[i] = s_gp[(bin0 + (unsigned)i) / kScanBins] + lrow[i] + row[i];
        const uint64_t r0 = ((uint64_t)plane * nblocks + lb) * (uint64_t)G.region;

        // A region that fits one sub-batch (the usual case) needs no counting pass: its per-tile counts are this K1
        // workgroup's histogram row, already in the packed layout of cnt (needs the unit's first bin word-aligned).
        const bool single = count <= (unsigned)kSortBatch && (((unsigned)plane * (unsigned)tpp) & 1u) == 0u;
        for (unsigned s0 = 0; s0 < count; s0 += kSortBatch) {
            const unsigned nsub = count - s0 < (unsigned)kSortBatch ? count - s0 : (unsigned)kSortBatch;
            if (!single) {
                for (int i = tid; i < tw; i += kSortBlock)
                    cnt[i] = 0;
                lds_barrier();
            }
            unsigned tile[R];
            float2 xy[R];
            float m[R];
#pragma unroll
            for (int k = 0; k < R; k++) {
                const unsigned i = (unsigned)k * kSortBlock + tid;
                if (i < nsub) {
                    tile[k] = cbin[r0 + s0 + i];
                    xy[k] = cxy[r0 + s0 + i];
                    if (HAS_MASS)
                        m[k] = cm[r0 + s0 + i];
                    if (!single)
                        atomicAdd(&cnt[tile[k] >> 1], 1u << ((tile[k] & 1u) * 16u));
                }
            }
            if (single) {
                const unsigned *hrow =
                    hist16w + (size_t)lb * (size_t)((G.nbins + 1) >> 1) + (((size_t)plane * tpp) >> 1);
                for (int i = tid; i < tw; i += kSortBlock)
                    cnt[i] = (i == tw - 1 && (tpp & 1)) ? (hrow[i] & 0xFFFFu) : hrow[i];
            }
            lds_barrier();
            // exclusive scan of cnt -> pos; lane handles tiles [tid*per, tid*per + per).  The cursor is stored minus
            // the tile's sorted start, so that the write-out needs a single table: dst = cur[t] + sorted position.
            {
                unsigned sum = 0;
                for (int j = 0; j < per; j++) {
                    const unsigned t = (unsigned)(tid * per + j);
                    if ((int)t < tpp)
                        sum += get16(cnt, t);
                }
                unsigned e = block_exclusive_scan(sum, s_wave);
                for (int j = 0; j < per; j++) {
                    const unsigned t = (unsigned)(tid * per + j);
                    if ((int)t < tpp) {
                        pos[t] = e;
                        cur[t] -= e;
                        e += get16(cnt, t);
                    }
                }
            }
            lds_barrier();
            // sorted position of every record (one returning LDS add), kept in the upper half of tile[]
#pragma unroll
            for (int k = 0; k < R; k++) {
                const unsigned i = (unsigned)k * kSortBlock + tid;
                if (i < nsub)
                    tile[k] |= atomicAdd(&pos[tile[k]], 1u) << 16;
                else
                    tile[k] = 0xFFFF0000u;  // position 65535: outside every staging round
            }
            if (HAS_MASS) {
#pragma unroll
                for (int k = 0; k < R; k++)
                    if ((unsigned)k * kSortBlock + tid < nsub)
                        mass_max = fmaxf(mass_max, cap_mass(m[k]));
            }
            // exchange through LDS and write out, kSortStage sorted positions at a time (the staging area is what
            // limits the workgroups per CU)
            for (unsigned lo = 0; lo < nsub; lo += kSortStage) {
                lds_barrier();  // positions final (first round) / previous round's staging consumed
#pragma unroll
                for (int k = 0; k < R; k++) {
                    const unsigned q = (tile[k] >> 16) - lo;
                    if (q < (unsigned)kSortStage) {
                        sorted_xy[q] = xy[k];
                        sorted_tile[q] = (unsigned short)(tile[k] & 0xFFFFu);
                        if (HAS_MASS)
                            sorted_m[q] = m[k];
                    }
                }
                lds_barrier();
                const unsigned hi = nsub - lo < (unsigned)kSortStage ? nsub - lo : (unsigned)kSortStage;
                for (unsigned q = tid; q < hi; q += kSortBlock) {
                    const unsigned dst = cur[sorted_tile[q]] + lo + q;
                    if (HAS_MASS) {  // one 12-byte record instead of an 8-byte and a 4-byte stream
                        const float2 v = sorted_xy[q];
                        reinterpret_cast<Rec3 *>(sxy)[dst] = Rec3{v.x, v.y, sorted_m[q]};
                    } else {
                        sxy[dst] = sorted_xy[q];
                    }
                }
            }
            if (!single) {
                lds_barrier();
                // next sub-batch: cursor = old cursor + count = (cursor - start) + (start + count) = cur + pos
                for (int i = tid; i < tpp; i += kSortBlock)
                    cur[i] += pos[i];
            }
        }
    }
    if (HAS_MASS) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1)
            mass_max = fmaxf(mass_max, __shfl_xor(mass_max, d));
        if (lane_id() == 0 && __float_as_uint(mass_max) > *T.max_mass)
            atomicMax(T.max_mass, __float_as_uint(mass_max));
    }
}

// ---------------------------------------------------------------------------------------------
// K3': second level of the two-level sort
// ---------------------------------------------------------------------------------------------
// The project+bin kernel (SORT2) leaves, per workgroup, sub-batches of records sorted by unit (coarse bin) with a table
// of where each unit's run starts.  One work item here = (unit, group of slots_per_group sub-batch slots = 16
// project+bin workgroups): it gathers the unit's runs of those sub-batches (contiguous pieces of ~0.5 KB), sorts the
// ~6000 records by tile-in-unit in LDS (counting sort over <= 256 tiles) and writes them as ONE contiguous piece of
// sxy, tile after tile, plus the item's row of ptab (where each tile's run starts).  Pieces are allocated with one
// atomic add per item; the tile kernel finds a tile's runs through ptab (build_run_table).  No global histogram, no
// prefix matrix, every store a run of >= ~0.4 KB.
constexpr int kS2Block = 512;
constexpr int kS2Cap = 8192;  // records sorted at a time (the LDS staging area); larger items take several windows
constexpr int kS2R = kS2Cap / kS2Block;
constexpr int kS2MaxMine = 64;  // items one persistent workgroup may have to take (host: nitems <= 64 * workgroups)

template <bool POW2>
__device__ __forceinline__ unsigned sort2_tile_of(float2 r, const PassParams &P, const BinGeom &G)
{
    const int nn = P.nn;
    int gx = grid_index<POW2>(r.x, P), gy = grid_index<POW2>(r.y, P);
    gx = min(max(gx, 0), nn - 1);  // (border-ring entries were binned with the clamped cell)
    gy = min(max(gy, 0), nn - 1);
    const unsigned ty = (unsigned)(gy >> G.th_log2), tx = (unsigned)(gx >> G.tw_log2);
    return (ty % (unsigned)G.rows_per_unit) * (unsigned)G.ntx + tx;
}

template <bool POW2>
__global__ __launch_bounds__(kS2Block, 4) void k_sort2(const float2 *__restrict__ c1, const unsigned *__restrict__ sb_off,
                                                       const unsigned short *__restrict__ sb_start,
                                                       const unsigned *__restrict__ sb_n, int nblocks, int slots_per_group,
                                                       int ngroups, BinGeom G, PassParams P, float2 *__restrict__ sxy,
                                                       unsigned *__restrict__ ptab, const unsigned *__restrict__ item_tot,
                                                       unsigned *tile_tot)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s2[];
    const int S = slots_per_group, ntc = G.tiles_per_unit;
    float2 *stage = reinterpret_cast<float2 *>(smem_s2);                      // [kS2Cap] records in sorted order
    unsigned char *scol = reinterpret_cast<unsigned char *>(stage + kS2Cap);  // [kS2Cap] tile-in-unit of stage[i]
    unsigned *r_src = reinterpret_cast<unsigned *>(scol + kS2Cap);            // [S] first record of run r in c1
    unsigned *r_off = r_src + S;                                              // [S + 1] runs concatenated: start of run r
    unsigned *cnt = r_off + S + 1;                                            // [ntc] records per tile (this window)
    unsigned *pos = cnt + ntc;                                                // [ntc] running sorted position (window)
    unsigned *adj = pos + ntc;  // [ntc] global position of the tile's first record of this window minus its sorted start
    unsigned *cur = adj + ntc;  // [ntc] records of the tile already written (+ its start inside the item)
    unsigned short *first = reinterpret_cast<unsigned short *>(cur + ntc);  // [kS2Cap / 64] run of the window's record 64 c
    __shared__ unsigned s_wave[kS2Block / 64];
    __shared__ unsigned s_mybase[kS2MaxMine];
    const int tid = threadIdx.x;
    const int nslots = nblocks * kSubBatches;
    const int nitems = G.n_units * ngroups;
    // Where this workgroup's items go in sxy: the exclusive prefix of the item totals (summed by the project+bin kernel),
    // in item order -- every workgroup scans the (<= 8192) totals once for itself; no allocation atomics, and the layout
    // of sxy does not depend on the order in which the items are processed.
    {
        const int per = (nitems + kS2Block - 1) / kS2Block;
        unsigned sum = 0;
        for (int j = 0; j < per; j++) {
            const int idx = tid * per + j;
            sum += idx < nitems ? item_tot[idx] : 0u;
        }
        unsigned e = block_exclusive_scan(sum, s_wave);
        for (int j = 0; j < per; j++) {
            const int idx = tid * per + j;
            if (idx < nitems) {
                const int rel = idx - (int)blockIdx.x;
                if (rel >= 0 && rel % (int)gridDim.x == 0)
                    s_mybase[rel / (int)gridDim.x] = e;
                e += item_tot[idx];
            }
        }
        lds_barrier();
    }
    // this thread's run of item `it`: (length, first record in c1); requested one item ahead, so that the two dependent
    // table reads of the next item travel while the current one is sorted
    auto item_run = [&](int it, unsigned &len, unsigned &src) {
        len = 0;
        src = 0;
        if (it >= nitems || tid >= S)
            return;
        const int g = it / G.n_units, b = it % G.n_units;
        const int sl = g * S + tid;
        if (sl < nslots) {
            const int w = sl / kSubBatches, f = sl % kSubBatches;
            if ((unsigned)f < sb_n[w]) {
                const unsigned a = sb_start[(size_t)sl * kSubRow + b], e = sb_start[(size_t)sl * kSubRow + b + 1];
                len = e - a;
                src = sb_off[sl] + a;
            }
        }
    };
    unsigned len_next, src_next;
    item_run(blockIdx.x, len_next, src_next);
    for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int g = it / G.n_units, b = it % G.n_units;  // (neighbouring items read neighbouring runs of the same sub-batches)
        const unsigned len = len_next, src = src_next;
        item_run(it + (int)gridDim.x, len_next, src_next);
        lds_barrier();  // the previous item's tables and staging are no longer read
        const unsigned off = block_exclusive_scan(len, s_wave);
        if (tid < S) {
            r_src[tid] = src;
            r_off[tid] = off;
        }
        if (tid == S - 1)
            r_off[S] = off + len;
        for (int i = tid; i < ntc; i += kS2Block)
            cnt[i] = 0;
        lds_barrier();
        const unsigned total = r_off[S];
        unsigned *prow = ptab + ((size_t)b * (size_t)ngroups + (size_t)g) * (size_t)(ntc + 1);
        // (an item whose runs do not add up to the total the project+bin kernel reported is dropped rather than
        // written over its neighbours: cannot happen unless the two kernels disagree, and then the parity tests see it)
        if (total == 0 || total != item_tot[it]) {  // (uniform)
            for (int i = tid; i <= ntc; i += kS2Block)
                prow[i] = 0;
            continue;
        }
        const unsigned s_base = s_mybase[(it - (int)blockIdx.x) / (int)gridDim.x];
        const bool multi = total > (unsigned)kS2Cap;
        // windows of kS2Cap records of the concatenated runs; pass 0 of a multi-window item only counts (the item's
        // tile starts must be known before its first record is placed)
        for (int pass = multi ? 0 : 1; pass < 2; pass++) {
            for (unsigned p0 = 0; p0 < total; p0 += kS2Cap) {
                const unsigned p1 = p0 + kS2Cap < total ? p0 + kS2Cap : total, nsub = p1 - p0;
                // run that holds the first record of every piece of 64 (binary search over the run starts)
                for (unsigned pc = tid; pc < (nsub + 63) >> 6; pc += kS2Block) {
                    const unsigned q = p0 + (pc << 6);
                    int lo = 0, hi = S - 1;  // largest r with r_off[r] <= q
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (r_off[mid] <= q)
                            lo = mid;
                        else
                            hi = mid - 1;
                    }
                    first[pc] = (unsigned short)lo;
                }
                lds_barrier();
                // gather: thread tid takes the window's records tid, tid + 512, ...: sixteen independent loads
                float2 rec[kS2R];
                unsigned sp[kS2R];
#pragma unroll
                for (int k = 0; k < kS2R; k++) {
                    const unsigned i = (unsigned)k * kS2Block + tid;
                    const unsigned q = p0 + (i < nsub ? i : nsub - 1);  // clamped: unconditional loads
                    int r = first[(q - p0) >> 6];
                    while (q >= r_off[r + 1])
                        r++;
                    rec[k] = c1[r_src[r] + (q - r_off[r])];
                }
#pragma unroll
                for (int k = 0; k < kS2R; k++) {
                    const unsigned i = (unsigned)k * kS2Block + tid;
                    sp[k] = 0xFFFFFFFFu;
                    if (i < nsub) {
                        sp[k] = sort2_tile_of<POW2>(rec[k], P, G);
                        atomicAdd(&cnt[sp[k]], 1u);
                    }
                }
                lds_barrier();
                const unsigned c = tid < ntc ? cnt[tid] : 0u;
                if (pass == 0) {  // counting pass: leave the counts, the item's tile starts follow after the last window
                    if (p1 < total)
                        continue;
                    const unsigned e = block_exclusive_scan(c, s_wave);
                    if (tid < ntc) {
                        cur[tid] = e;  // start of the tile's records inside the item
                        prow[tid] = s_base + e;
                        cnt[tid] = 0;
                    }
                    if (tid == 0)
                        prow[ntc] = s_base + total;
                    lds_barrier();
                    continue;
                }
                const unsigned e = block_exclusive_scan(c, s_wave);
                if (tid < ntc) {
                    unsigned at;  // start of this window's records of the tile inside the item
                    if (multi) {
                        at = cur[tid];
                    } else {
                        at = e;
                        prow[tid] = s_base + e;
                    }
                    pos[tid] = e;
                    adj[tid] = s_base + at - e;
                    cur[tid] = at + c;
                    cnt[tid] = 0;
                    if (c)
                        atomicAdd(&tile_tot[(size_t)b * ntc + tid], c);
                }
                if (!multi && tid == 0)
                    prow[ntc] = s_base + total;
                lds_barrier();
#pragma unroll
                for (int k = 0; k < kS2R; k++)
                    if (sp[k] != 0xFFFFFFFFu) {
                        const unsigned t = sp[k], at = atomicAdd(&pos[t], 1u);
                        stage[at] = rec[k];
                        scol[at] = (unsigned char)t;
                    }
                lds_barrier();
                for (unsigned i = tid; i < nsub; i += kS2Block)
                    sxy[adj[scol[i]] + i] = stage[i];
                if (p1 < total)
                    lds_barrier();  // the next window overwrites the staging area
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
hipError_t launch_bin_scan(const LaunchCfg &cfg, int nblocks, int n_planes, const BinGeom &G, const BinWorkspace &W,
                           const Targets &T, hipStream_t s)
{
    (void)cfg, (void)n_planes, (void)T;
    const int ngroups = (G.nbins + kScanBins - 1) / kScanBins;
    k_scan_blocks<<<ngroups, 1024, 0, s>>>(reinterpret_cast<const unsigned short *>(W.hist16), W.hist, W.total,
                                           W.total + kMaxBins, nblocks, G.nbins);
    return hipGetLastError();
}

size_t scatter_lds_bytes(const BinGeom &G, bool has_mass)
{
    const size_t tpp = (size_t)G.tiles_per_unit, tw = (tpp + 1) >> 1;
    return 4 * (tw + 2 * tpp + (tw & 1)) + (size_t)kSortStage * (8 + 2 + (has_mass ? 4 : 0));
}

hipError_t launch_bin_scatter(const LaunchCfg &cfg, int nblocks, int n_planes, int max_workgroups, const BinGeom &G,
                              const BinWorkspace &W, const Targets &T, hipStream_t s)
{
    const bool has_mass = cfg.has_mass;
    const size_t lds = scatter_lds_bytes(G, has_mass);
    const int items = G.n_units * 8 * ((nblocks + 7) / 8);
    const int nwg = std::min(items, std::max(8, max_workgroups / 8 * 8));
    const int count_planes = n_planes;  // records per plane -> selected-entry counters (NGP adds its dropped ones in K1)
    return launch_with_lds(has_mass ? k_bin_scatter<true> : k_bin_scatter<false>, nwg, kSortBlock, lds, /*raise_above=*/0, s,
                           W.cxy, W.cbin, W.cm, W.hist16, W.hist, W.total, W.total + kMaxBins, W.base, W.bcount, nblocks, G,
                           W.sxy, W.sm, count_planes, T);
}

size_t sort2_lds_bytes(int slots_per_group, int tiles_per_unit)
{
    return (size_t)kS2Cap * 9 + 4 * ((size_t)slots_per_group * 2 + 1 + 4 * (size_t)tiles_per_unit) + 2 * (kS2Cap / 64);
}

hipError_t launch_sort2(int nblocks, int slots_per_group, int ngroups, int max_workgroups, const PassParams &P,
                        const BinGeom &G, const BinWorkspace &W, hipStream_t s)
{
    const size_t lds = sort2_lds_bytes(slots_per_group, G.tiles_per_unit);
    const int nitems = G.n_units * ngroups;
    const int nwg = std::min(nitems, std::max(std::max(8, max_workgroups), (nitems + kS2MaxMine - 1) / kS2MaxMine));
    return launch_with_lds(P.pow2 ? k_sort2<true> : k_sort2<false>, nwg, kS2Block, lds, /*raise_above=*/0, s, W.c1, W.sb_off,
                           W.sb_start, W.sb_n, nblocks, slots_per_group, ngroups, G, P, W.sxy, W.ptab, W.item_tot, W.tot);
}

}  // namespace slicer
