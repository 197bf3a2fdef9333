// slicer_catalogue.hip -- on-device catalogue of a map's peaks and minima: where they are, how high, and a sub-pixel
// offset from a quadratic fit.
//
// Of an n x n f32 map x (row-major, only read): the pixels 1 <= i, j <= n-2 strictly greater (peaks) or strictly less
// (minima) in f32 than each of their 8 neighbours -- the rule of slicer_peaks.hip (row N10): ties give neither, a
// comparison with a NaN is false, nothing wraps -- that pass the selection of the run: a peak iff (double)x >= min_peak,
// a minimum iff (double)x <= max_minimum, each kind only if its bit of `kinds` is set.  One record of 32 bytes a kept
// pixel (slicer_catalogue_record), in ascending i * n + j, the first `capacity` of them; the totals by kind are exact
// whatever the capacity.
// The compaction has no atomics and no workgroup waits on another: three steps, each a launch of its own.
//   k_catalogue<false>  count.  The tile, its LDS window and the two load paths are those of k_peaks: 16 x 64 pixels
//                       with a halo of one, rows of pitch 72, a float4 per four pixels when 4 | n and the map is on the
//                       16-byte grid, scalar loads otherwise.  After staging, wave w of the workgroup takes rows 4 w ...
//                       4 w + 3 of the tile and lane l column l of each: the 64 pixels of one row of a tile -- a segment
//                       -- are one wave's, so a ballot of `kept` is the segment's bitmap and its population count the
//                       segment's count.  Lane 0 stores seg[i * tiles_x + tx] = kept | kept minima << 16: the segments
//                       in index order are the pixels in record order.  Every segment of the map is stored by every
//                       launch: nothing is zeroed between runs and nothing carried over.
//   k_block_sums, k_top, k_block_offsets
//                       scan.  Blocks of 4096 segments: their sums (kept, kept minima); one workgroup turns the at most
//                       4096 block sums into exclusive offsets and stores the totals {peaks, minima, stored} as int64;
//                       every block then overwrites its segments' counts with their exclusive offsets.  All u32: there
//                       are at most n^2 / 4 peaks and as many minima (no two of a kind are adjacent), 2^29 together at
//                       n = 32768.
//   k_catalogue<true>   emit.  The same window, the same test, the same ballot; a kept pixel's record goes to
//                       seg[...] + (the kept pixels of its segment in lower lanes) if that is below the capacity, as two
//                       16-byte stores.  The map is read twice instead of keeping a flag per pixel.
// The record's position depends on the map alone -- not on the grid, the number of CUs or the load path -- and the
// refinement is plain f64 arithmetic in a stated order (-ffp-contract=off: no fused multiply-add), so every byte is the
// same on every run.
#include <hip/hip_runtime.h>

#include "slicer_rank_counts.hpp"

namespace {

constexpr int kRows = kT0 + 2;                      // window rows: the tile and its halo
constexpr int kCatMaxNpix = SLICER_CATALOGUE_MAX_NPIX;
constexpr int64_t kCatMaxCapacity = SLICER_CATALOGUE_MAX_CAPACITY;
constexpr int kWave = 64, kWaves = kThreads / kWave, kRowsPerWave = kT0 / kWaves;
constexpr int kScanPer = 16, kScanItems = kThreads * kScanPer;  // segments of a thread, of a block of the scan
constexpr int kMaxScanBlocks = kScanItems;                      // k_top is one workgroup: a thread takes kScanPer block sums

static_assert(kT1 == kWave && kRowsPerWave * kWaves == kT0, "a segment -- one row of a tile -- is one wave64 of pixels");
static_assert(sizeof(slicer_catalogue_record) == 32 && alignof(slicer_catalogue_record) == 8, "a record is two 16-byte stores");
static_assert((int64_t)kCatMaxNpix * kCatMaxNpix / 2 <= kCatMaxCapacity && kCatMaxCapacity < (int64_t)1 << 32,
              "u32 offsets hold every record: at most n^2 / 4 peaks and n^2 / 4 minima");
static_assert(((int64_t)kCatMaxNpix * (kCatMaxNpix / kT1) + kScanItems - 1) / kScanItems <= kMaxScanBlocks,
              "one workgroup scans the block sums of the largest map");
static_assert(kT1 < 1 << 16, "a segment's two counts share a u32");

struct CatArgs {
    const float *x;
    unsigned *seg;                     // [n * tiles_x]: count: kept | kept minima << 16; emit: the exclusive offsets
    slicer_catalogue_record *records;  // [capacity]
    double min_peak, max_minimum;
    unsigned capacity;
    int n, kinds;
    int tiles_x, ntiles;
};

// The window of the tile at (r0, c0), as k_peaks stages it: zeros outside the map (no candidate has a neighbour there).
template <bool VEC>
__device__ __forceinline__ void stage_window(float *win, const float *x, int n, int r0, int c0)
{
    const int tid = threadIdx.x;
    if (VEC) {  // 4 | n and c0 % 4 == 0: a float4 lies in the map whole or not at all
        for (int q = tid; q < kRows * kQuads; q += kThreads) {
            const int wr = q / kQuads, wq = q % kQuads;
            const int r = r0 - 1 + wr, c = c0 + kPer * wq;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r >= 0 && r < n && c < n)
                v = *reinterpret_cast<const float4 *>(x + (size_t)r * n + c);
            *reinterpret_cast<float4 *>(win + wr * kPitch + kLeft + kPer * wq) = v;
        }
        if (tid < 2 * kRows) {  // the two halo columns
            const int wr = tid / 2, right = tid % 2;
            const int r = r0 - 1 + wr, c = right ? c0 + kT1 : c0 - 1;
            win[wr * kPitch + (right ? kLeft + kT1 : kLeft - 1)] = r >= 0 && r < n && c >= 0 && c < n ? x[(size_t)r * n + c] : 0.0f;
        }
    } else {
        for (int q = tid; q < kRows * (kT1 + 2); q += kThreads) {
            const int wr = q / (kT1 + 2), wc = q % (kT1 + 2);
            const int r = r0 - 1 + wr, c = c0 - 1 + wc;
            win[wr * kPitch + kLeft - 1 + wc] = r >= 0 && r < n && c >= 0 && c < n ? x[(size_t)r * n + c] : 0.0f;
        }
    }
}

// The least-squares quadratic of the 3 x 3 window z[a + 1][b + 1] (a the row offset, b the column offset), every value
// widened exactly to f64, every operation rounded once, in the order of the contract (include/slicer_amd.h).  Returns
// the record's flags; dy = dx = +0.0 where the offsets are not accepted.
__device__ __forceinline__ unsigned refine(const float (&zf)[3][3], bool minimum, double &dy, double &dx)
{
    double z[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++)
            z[a][b] = (double)zf[a][b];
    double R[3], Cs[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        R[k] = (z[k][0] + z[k][1]) + z[k][2];
        Cs[k] = (z[0][k] + z[1][k]) + z[2][k];
    }
    const double gy = (R[2] - R[0]) / 6.0, gx = (Cs[2] - Cs[0]) / 6.0;
    const double hyy = ((R[2] + R[0]) - 2.0 * R[1]) / 3.0, hxx = ((Cs[2] + Cs[0]) - 2.0 * Cs[1]) / 3.0;
    const double hxy = ((z[2][2] + z[0][0]) - (z[2][0] + z[0][2])) / 4.0;
    const double det = hyy * hxx - hxy * hxy;
    const double oy = -((hxx * gy - hxy * gx) / det), ox = -((hyy * gx - hxy * gy) / det);
    const bool curved = minimum ? hyy > 0.0 : hyy < 0.0;
    // (a NaN or an infinite offset fails the last two comparisons)
    const bool ok = det > 0.0 && curved && fabs(oy) <= 0.5 && fabs(ox) <= 0.5;
    dy = ok ? oy : 0.0;
    dx = ok ? ox : 0.0;
    return (minimum ? SLICER_CATALOGUE_MINIMUM : 0u) | (ok ? 0u : SLICER_CATALOGUE_FALLBACK);
}

template <bool VEC, bool EMIT>
__global__ __launch_bounds__(kThreads) void k_catalogue(CatArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kRows * kPitch];
    const int n = a.n, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const bool want_peaks = a.kinds & SLICER_CATALOGUE_PEAKS, want_minima = a.kinds & SLICER_CATALOGUE_MINIMA;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int tx = t % a.tiles_x, r0 = t / a.tiles_x * kT0, c0 = tx * kT1;
        __syncthreads();  // the previous tile's window has been read
        stage_window<VEC>(win, a.x, n, r0, c0);
        __syncthreads();
        const int j = c0 + lane;
        // rows i-1 ... i+1 of the wave's kRowsPerWave rows i, columns j-1 ... j+1
        const float *w = win + wave * kRowsPerWave * kPitch + kLeft + lane;
        float z[kRowsPerWave + 2][3];
#pragma unroll
        for (int d = 0; d < kRowsPerWave + 2; d++)
#pragma unroll
            for (int b = 0; b < 3; b++)
                z[d][b] = w[d * kPitch + b - 1];
#pragma unroll
        for (int k = 0; k < kRowsPerWave; k++) {
            const int i = r0 + wave * kRowsPerWave + k;
            if (i >= n)
                break;  // (the same for the whole wave)
            const float c = z[k + 1][1];
            bool peak = true, minimum = true;
#pragma unroll
            for (int d = 0; d < 3; d++)
#pragma unroll
                for (int b = 0; b < 3; b++)
                    if (d != 1 || b != 1) {
                        peak = peak && c > z[k + d][b];
                        minimum = minimum && c < z[k + d][b];
                    }
            const bool inside = i >= 1 && i <= n - 2 && j >= 1 && j <= n - 2;
            peak = peak && inside && want_peaks && (double)c >= a.min_peak;
            minimum = minimum && inside && want_minima && (double)c <= a.max_minimum;
            const unsigned long long kept = __ballot(peak || minimum);
            const size_t s = (size_t)i * a.tiles_x + tx;
            if (!EMIT) {
                const unsigned long long minima = __ballot(minimum);
                if (lane == 0)
                    a.seg[s] = (unsigned)__popcll(kept) | (unsigned)__popcll(minima) << 16;
                continue;
            }
            if (!(peak || minimum))
                continue;
            const unsigned at = a.seg[s] + (unsigned)__popcll(kept & ((1ull << lane) - 1ull));
            if (at >= a.capacity)
                continue;
            const float zz[3][3] = {{z[k][0], z[k][1], z[k][2]},
                                    {z[k + 1][0], z[k + 1][1], z[k + 1][2]},
                                    {z[k + 2][0], z[k + 2][1], z[k + 2][2]}};
            double dy, dx;
            const unsigned flags = refine(zz, minimum, dy, dx);
            uint4 head;
            head.x = (unsigned)i, head.y = (unsigned)j, head.z = __float_as_uint(c), head.w = flags;
            uint4 *out = reinterpret_cast<uint4 *>(a.records + at);
            out[0] = head;
            *reinterpret_cast<double2 *>(out + 1) = make_double2(dy, dx);
        }
    }
}

// Exclusive sums of one value a thread over the workgroup (Hillis-Steele in LDS); *total: the sum of all.
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned *lds, unsigned *total)
{
    const int tid = threadIdx.x;
    __syncthreads();  // an earlier call's reads
    lds[tid] = v;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const unsigned below = tid >= d ? lds[tid - d] : 0u;
        __syncthreads();
        lds[tid] += below;
        __syncthreads();
    }
    *total = lds[kThreads - 1];
    return lds[tid] - v;
}

// bsum[b] = (the kept pixels, the kept minima) of the segments b * kScanItems ... of seg[nseg]
__global__ __launch_bounds__(kThreads) void k_block_sums(const unsigned *seg, int nseg, uint2 *bsum)
{
    __shared__ unsigned lds[kThreads];
    const int first = (int)blockIdx.x * kScanItems + (int)threadIdx.x * kScanPer;
    unsigned kept = 0, minima = 0;
    for (int e = 0; e < kScanPer && first + e < nseg; e++) {
        const unsigned w = seg[first + e];
        kept += w & 0xffffu;
        minima += w >> 16;
    }
    unsigned all_kept, all_minima;
    block_exclusive(kept, lds, &all_kept);
    block_exclusive(minima, lds, &all_minima);
    if (threadIdx.x == 0)
        bsum[blockIdx.x] = make_uint2(all_kept, all_minima);
}

// One workgroup: boff[b] = the kept pixels of the blocks before b; totals = {peaks, minima, stored}
__global__ __launch_bounds__(kThreads) void k_top(const uint2 *bsum, int nb, unsigned *boff, int64_t *totals, unsigned capacity)
{
    __shared__ unsigned lds[kThreads];
    const int first = (int)threadIdx.x * kScanPer;
    unsigned kept = 0, minima = 0;
    for (int e = 0; e < kScanPer && first + e < nb; e++) {
        kept += bsum[first + e].x;
        minima += bsum[first + e].y;
    }
    unsigned all_kept, all_minima;
    unsigned at = block_exclusive(kept, lds, &all_kept);
    block_exclusive(minima, lds, &all_minima);
    for (int e = 0; e < kScanPer && first + e < nb; e++) {
        boff[first + e] = at;
        at += bsum[first + e].x;
    }
    if (threadIdx.x == 0) {
        totals[0] = (int64_t)(all_kept - all_minima);
        totals[1] = (int64_t)all_minima;
        totals[2] = (int64_t)(all_kept < capacity ? all_kept : capacity);
    }
}

// seg[s]: from the segment's counts to the kept pixels of all segments before s
__global__ __launch_bounds__(kThreads) void k_block_offsets(unsigned *seg, int nseg, const unsigned *boff)
{
    __shared__ unsigned lds[kThreads];
    const int first = (int)blockIdx.x * kScanItems + (int)threadIdx.x * kScanPer;
    unsigned cnt[kScanPer], kept = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; e++) {
        cnt[e] = first + e < nseg ? seg[first + e] & 0xffffu : 0u;
        kept += cnt[e];
    }
    unsigned all_kept;
    unsigned at = boff[blockIdx.x] + block_exclusive(kept, lds, &all_kept);
#pragma unroll
    for (int e = 0; e < kScanPer; e++) {
        if (first + e < nseg)
            seg[first + e] = at;
        at += cnt[e];
    }
}

const char *const kCreate = "slicer_catalogue_create";

}  // namespace

struct slicer_catalogue : SubHandle {
    int n = 0;     // the largest map side
    int gmax = 0;  // workgroups of k_catalogue at most
    int64_t capacity = 0;
    slicer_catalogue_record *records = nullptr;  // the handle's own, or the caller's
    unsigned *seg = nullptr, *boff = nullptr;
    uint2 *bsum = nullptr;
    int64_t *totals = nullptr;  // peaks, minima, stored
    bool ran = false;
};

// What a run refuses before it looks at its handle, in this order: the kinds, a NaN threshold; then a missing handle or map.
static int run_refusal(const slicer_catalogue *ch, const float *d_map, int32_t kinds, double min_peak, double max_minimum,
                       const char *who)
{
    slicer_handle h = ch ? ch->h : nullptr;
    if (kinds < 1 || kinds > (SLICER_CATALOGUE_PEAKS | SLICER_CATALOGUE_MINIMA))
        return fail(h, SLICER_ERR_ARG, "%s: kinds = %d outside 1..3", who, kinds);
    if (min_peak != min_peak || max_minimum != max_minimum)
        return fail(h, SLICER_ERR_ARG, "%s: a threshold is NaN", who);
    if (!ch || !d_map)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    return SLICER_OK;
}

extern "C" {

int slicer_catalogue_create(slicer_handle h, int32_t npix, int64_t capacity, void *d_records, slicer_catalogue_handle *out)
{
    if (out)
        *out = nullptr;
    // the numbers first: they need no handle, so a caller can have them checked before any device exists
    if (int rc = npix_in_range(h, kCreate, npix, kCatMaxNpix))
        return rc;
    if (capacity < 1 || capacity > kCatMaxCapacity)
        return fail(h, SLICER_ERR_ARG, "%s: capacity = %lld outside 1..%lld", kCreate, (long long)capacity,
                    (long long)kCatMaxCapacity);
    if ((uintptr_t)d_records % 16 != 0)
        return fail(h, SLICER_ERR_ARG, "%s: the records are off the 16-byte grid", kCreate);
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", kCreate);
    hipStream_t st = nullptr;
    slicer_catalogue_handle ch = nullptr;
    if (int rc = sub_new(h, kCreate, &st, &ch))
        return rc;
    ch->n = npix;
    ch->capacity = capacity;
    ch->gmax = resident_groups(kRows * kPitch * sizeof(float), tiles_of(npix), h->num_cus);
    const size_t nseg = (size_t)npix * tiles_across(npix), nb = (nseg + kScanItems - 1) / kScanItems;
    int rc = SLICER_OK;
    ch->records = static_cast<slicer_catalogue_record *>(d_records);
    if (!d_records)
        rc = ch->mem.alloc(rc, h, kCreate, (void **)&ch->records, (size_t)capacity * sizeof(slicer_catalogue_record));
    rc = ch->mem.alloc(rc, h, kCreate, (void **)&ch->seg, nseg * sizeof(unsigned));
    rc = ch->mem.alloc(rc, h, kCreate, (void **)&ch->bsum, nb * sizeof(uint2));
    rc = ch->mem.alloc(rc, h, kCreate, (void **)&ch->boff, nb * sizeof(unsigned));
    rc = ch->mem.alloc(rc, h, kCreate, (void **)&ch->totals, 3 * sizeof(int64_t));
    return sub_done(rc, ch, out);
}

int slicer_catalogue_run_npix(slicer_catalogue_handle ch, const float *d_map, int32_t kinds, double min_peak,
                              double max_minimum, int32_t npix)
{
    const char *who = "slicer_catalogue_run_npix";
    if (int rc = run_refusal(ch, d_map, kinds, min_peak, max_minimum, who))
        return rc;
    slicer_handle h = ch->h;
    if (npix < 1 || npix > ch->n)
        return fail(h, SLICER_ERR_ARG, "%s: npix = %d outside 1..%d", who, npix, ch->n);
    hipStream_t st;
    if (int rc = sub_stream(h, ch->device, &st))
        return rc;
    ch->ran = false;
    CatArgs a{};
    a.x = d_map;
    a.seg = ch->seg;
    a.records = ch->records;
    a.min_peak = min_peak;
    a.max_minimum = max_minimum;
    a.capacity = (unsigned)ch->capacity;
    a.n = npix;
    a.kinds = kinds;
    a.tiles_x = tiles_across(npix);
    a.ntiles = (int)tiles_of(npix);
    const int nseg = npix * a.tiles_x, nb = (nseg + kScanItems - 1) / kScanItems;
    const dim3 grid((unsigned)std::min(a.ntiles, ch->gmax)), block(kThreads);
    const bool vec = quads_aligned(d_map, npix);
    if (vec)
        hipLaunchKernelGGL((k_catalogue<true, false>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_catalogue<false, false>), grid, block, 0, st, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_block_sums, dim3((unsigned)nb), block, 0, st, ch->seg, nseg, ch->bsum);
    hipLaunchKernelGGL(k_top, dim3(1), block, 0, st, ch->bsum, nb, ch->boff, ch->totals, a.capacity);
    hipLaunchKernelGGL(k_block_offsets, dim3((unsigned)nb), block, 0, st, ch->seg, nseg, ch->boff);
    HIPCHK(h, hipGetLastError());
    if (vec)
        hipLaunchKernelGGL((k_catalogue<true, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_catalogue<false, true>), grid, block, 0, st, a);
    HIPCHK(h, hipGetLastError());
    ch->ran = true;
    return SLICER_OK;
}

int slicer_catalogue_run(slicer_catalogue_handle ch, const float *d_map, int32_t kinds, double min_peak, double max_minimum)
{
    if (int rc = run_refusal(ch, d_map, kinds, min_peak, max_minimum, "slicer_catalogue_run"))
        return rc;
    return slicer_catalogue_run_npix(ch, d_map, kinds, min_peak, max_minimum, ch->n);
}

int slicer_catalogue_count(slicer_catalogue_handle ch, int64_t *n_peaks, int64_t *n_minima, int64_t *stored)
{
    if (!ch)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_catalogue_count: null handle");
    if (!ch->ran)
        return fail(ch->h, SLICER_ERR_STATE, "slicer_catalogue_count before any slicer_catalogue_run");
    int64_t t[3];
    if (int rc = sub_read(*ch, t, ch->totals, sizeof t))
        return rc;
    if (n_peaks)
        *n_peaks = t[0];
    if (n_minima)
        *n_minima = t[1];
    if (stored)
        *stored = t[2];
    return SLICER_OK;
}

int slicer_catalogue_read(slicer_catalogue_handle ch, slicer_catalogue_record *records, int64_t max_records, int64_t *copied)
{
    if (!ch)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_catalogue_read: null handle");
    if (copied)
        *copied = 0;
    if (!ch->ran)
        return fail(ch->h, SLICER_ERR_STATE, "slicer_catalogue_read before any slicer_catalogue_run");
    if (max_records < 0 || (max_records > 0 && !records))
        return fail(ch->h, SLICER_ERR_ARG, "slicer_catalogue_read: %lld records into a %s array", (long long)max_records,
                    records ? "given" : "null");
    int64_t stored = 0;
    if (int rc = slicer_catalogue_count(ch, nullptr, nullptr, &stored))
        return rc;
    const int64_t take = std::min(stored, max_records);
    if (take > 0)
        if (int rc = sub_read(*ch, records, ch->records, (size_t)take * sizeof *records))
            return rc;
    if (copied)
        *copied = take;
    return SLICER_OK;
}

int slicer_catalogue_device(slicer_catalogue_handle ch, slicer_catalogue_record **d_records, int64_t **d_counts)
{
    if (!ch)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_catalogue_device: null handle");
    if (!ch->ran)
        return fail(ch->h, SLICER_ERR_STATE, "slicer_catalogue_device before any slicer_catalogue_run");
    if (d_records)
        *d_records = ch->records;
    if (d_counts)
        *d_counts = ch->totals;
    return SLICER_OK;
}

int slicer_catalogue_destroy(slicer_catalogue_handle ch) { return sub_destroy(ch); }

}  // extern "C"
