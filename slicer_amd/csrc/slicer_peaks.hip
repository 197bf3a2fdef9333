// slicer_peaks.hip -- on-device one-point PDF histogram and peak / minimum counts of a map.
//
// Of an n x n f32 map x (row-major, only read) and f64 edges e_0 < ... < e_B:
//   pdf[b]     pixels with e_b <= (double)x < e_{b+1}, the last bin closed (x = e_B is in bin B-1): numpy.histogram's rule;
//              below: x < e_0 or -inf; above: x > e_B or +inf; nan: NaN.  The comparisons are in f64 against the f64 edges.
//   peaks[b]   pixels 1 <= i, j <= n-2 strictly greater (in f32) than each of their 8 neighbours, binned by their own
//   minima[b]  value by the same rule; ... strictly less.  The map does not wrap: border pixels are never candidates.
//              A comparison with a NaN is false, so a NaN and its neighbours are neither; ties give neither.
// Every count is an integer: nothing here is a floating-point sum, so the results are exact and the same on every run.
//
// The tile, the search, the PDF rule, the grid size, the column sums and the host side of the entry points are those of
// slicer_rank_counts.hpp.
// k_peaks: a workgroup of 256 threads takes tiles of kT0 x kT1 = 16 x 64 pixels, stages a
// tile with a halo of one pixel in LDS as f32 and every thread takes four adjacent pixels of one row.  The window is
// 18 rows of pitch 72 with the tile's first column at window column 4 (not 18 x 66): the sixteen float4s of a window row
// then sit on LDS's 16-byte grid, so staging stores and a thread's three row reads are 128-bit accesses; the halo
// columns are window columns 3 and 68.  Loads: a float4 per four pixels when 4 | n and the map is on the 16-byte grid
// (k_peaks<true>), scalar loads otherwise (k_peaks<false>); the window, and so the counts, are the same.
// The grid is fixed: G = min(tiles, max(kMinGroups, w * CUs)) workgroups, w = min(8, what a CU's LDS holds at once),
// workgroup b takes tiles b, b + G, ..., so a workgroup zeroes and flushes its counters once a launch.  The edges sit
// in LDS as f64 (at most 8200 B); the bin is the number of e_0 ... e_{B-1} that are <= x, minus one, by rank_search
// over a thread's four pixels side by side; e_B only decides `above`, which closes the last bin.
// The counters are three u32 histograms of B bins and the 7 outside counts in LDS
// (at most 12316 B), incremented with LDS integer atomics; peaks and minima reuse the pixel's bin.
// u32 is enough: a workgroup counts at most ceil(tiles / G) * 1024 pixels, and tiles <= (131072 / 16) * (131072 / 64)
// = 2^24 with G >= min(tiles, 64) gives at most 2^18 * 2^10 = 2^28 < 2^32.
// Flush: workgroup b stores its counters as row b of partial[G][3 B + 7]; k_column_sums sums the rows of every column
// into int64.  Every row and every result is stored by every launch: nothing is zeroed between runs, nothing carried
// over, no global atomics.
#include <hip/hip_runtime.h>

#include "slicer_rank_counts.hpp"

namespace {

constexpr int kRows = kT0 + 2;  // window rows: the tile and its halo
constexpr int kMaxBins = SLICER_PEAKS_MAX_BINS;
constexpr int kOutside = 7;  // below[3], above[3], nan

static_assert(((int64_t)kMaxNpix / kT0) * (kMaxNpix / kT1) / kMinGroups * (kT0 * kT1) < (int64_t)1 << 32,
              "a workgroup's u32 counters hold every pixel it can meet");

struct PeakArgs {
    const float *x;
    const double *edges;  // [B + 1]
    unsigned *partial;    // [gridDim.x][3 B + 7]
    int n, B;
    int tiles_x, ntiles;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_peaks(PeakArgs a)
{
    __shared__ __attribute__((aligned(16))) float win[kRows * kPitch];
    extern __shared__ double dyn[];
    const int n = a.n, B = a.B, nE = B + 1, nC = 3 * B + kOutside, tid = threadIdx.x;
    double *edge = dyn;
    unsigned *cnt = reinterpret_cast<unsigned *>(dyn + nE);
    stage_table<kThreads>(edge, a.edges, nE);
    for (int k = tid; k < nC; k += kThreads)
        cnt[k] = 0u;
    const double eB = a.edges[B];
    const int lr = tid / kQuads, lc = tid % kQuads * kPer;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int r0 = t / a.tiles_x * kT0, c0 = t % a.tiles_x * kT1;
        __syncthreads();  // the previous tile's window has been read (first tile: edges and counters are in place)
        if (VEC) {        // 4 | n and c0 % 4 == 0: a float4 lies in the map whole or not at all
            for (int q = tid; q < kRows * kQuads; q += kThreads) {
                const int wr = q / kQuads, wq = q % kQuads;
                const int r = r0 - 1 + wr, c = c0 + kPer * wq;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (r >= 0 && r < n && c < n)
                    v = *reinterpret_cast<const float4 *>(a.x + (size_t)r * n + c);
                *reinterpret_cast<float4 *>(win + wr * kPitch + kLeft + kPer * wq) = v;
            }
            if (tid < 2 * kRows) {  // the two halo columns
                const int wr = tid / 2, right = tid % 2;
                const int r = r0 - 1 + wr, c = right ? c0 + kT1 : c0 - 1;
                win[wr * kPitch + (right ? kLeft + kT1 : kLeft - 1)] =
                    r >= 0 && r < n && c >= 0 && c < n ? a.x[(size_t)r * n + c] : 0.0f;
            }
        } else {
            for (int q = tid; q < kRows * (kT1 + 2); q += kThreads) {
                const int wr = q / (kT1 + 2), wc = q % (kT1 + 2);
                const int r = r0 - 1 + wr, c = c0 - 1 + wc;
                win[wr * kPitch + kLeft - 1 + wc] = r >= 0 && r < n && c >= 0 && c < n ? a.x[(size_t)r * n + c] : 0.0f;
            }
        }
        __syncthreads();
        const int i = r0 + lr, j0 = c0 + lc;
        if (i >= n || j0 >= n)
            continue;
        // rows i-1, i, i+1, columns j0-1 ... j0+4 of the map
        const float *w = win + (lr + 1) * kPitch + kLeft + lc;
        float nb[3][kPer + 2];
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const float *row = w + (d - 1) * kPitch;
            const float4 m = *reinterpret_cast<const float4 *>(row);
            nb[d][0] = row[-1];
            nb[d][1] = m.x, nb[d][2] = m.y, nb[d][3] = m.z, nb[d][4] = m.w;
            nb[d][5] = row[kPer];
        }
        // pos[q]: how many of e_0 ... e_{B-1} are <= pixel q.  (Pixels past the map's edge are zeros of the window:
        // searched, never counted.)
        double xd[kPer];
        int pos[kPer];
#pragma unroll
        for (int q = 0; q < kPer; q++)
            xd[q] = (double)nb[1][q + 1];
        rank_search(edge, B, xd, pos);
        const bool row_inside = i >= 1 && i <= n - 2;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int j = j0 + q;
            if (j >= n)
                break;
            const float x = nb[1][q + 1];
            // the pdf's counter of this pixel, and the distance from it to the peaks' one (the minima's: twice that)
            const int slot = pdf_slot(xd[q], pos[q], eB, 3 * B, 3), stride = slot < B ? B : 1;  // below[3], above[3], nan
            atomicAdd(&cnt[slot], 1u);
            if (slot == 3 * B + 6)
                continue;  // a NaN: every comparison with it is false, neither a peak nor a minimum
            if (!row_inside || j < 1 || j > n - 2)
                continue;
            const float c00 = nb[0][q], c01 = nb[0][q + 1], c02 = nb[0][q + 2], c10 = nb[1][q], c12 = nb[1][q + 2];
            const float c20 = nb[2][q], c21 = nb[2][q + 1], c22 = nb[2][q + 2];
            const bool peak = x > c00 && x > c01 && x > c02 && x > c10 && x > c12 && x > c20 && x > c21 && x > c22;
            const bool minimum = x < c00 && x < c01 && x < c02 && x < c10 && x < c12 && x < c20 && x < c21 && x < c22;
            if (peak)
                atomicAdd(&cnt[slot + stride], 1u);
            if (minimum)
                atomicAdd(&cnt[slot + 2 * stride], 1u);
        }
    }
    __syncthreads();
    unsigned *out = a.partial + (size_t)blockIdx.x * nC;
    for (int k = tid; k < nC; k += kThreads)
        out[k] = cnt[k];
}

size_t peaks_dyn_lds(int B) { return (size_t)(B + 1) * sizeof(double) + (3 * (size_t)B + kOutside) * sizeof(unsigned); }

const RankModule kPeaks = {"slicer_peaks", "slicer_peaks_create", "edges", "fewer than 2 edges", 2, kMaxBins + 1, kMaxNpix};

}  // namespace

struct slicer_peaks : RankHandle {  // table: the B + 1 edges
    int B = 0;
    unsigned *partial = nullptr;
    int64_t *res = nullptr;
};

extern "C" {

int slicer_peaks_edges(double lo, double hi, int32_t bins, double *edges)
{
    if (bins < 1 || bins > kMaxBins)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_peaks_edges: bins = %d outside 1..%d", bins, kMaxBins);
    if (!edges)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_peaks_edges: null argument");
    if (!std::isfinite(lo) || !std::isfinite(hi))
        return fail(nullptr, SLICER_ERR_ARG, "slicer_peaks_edges: lo and hi must be finite");
    const double width = (hi - lo) / (double)bins;
    edges[0] = lo;
    for (int b = 1; b < bins; b++)
        edges[b] = lo + (double)b * width;  // (-ffp-contract=off: the product and the sum are rounded apart)
    edges[bins] = hi;
    if (ascending_fault(bins + 1, edges))
        return fail(nullptr, SLICER_ERR_ARG,
                    "slicer_peaks_edges: the edges of lo = %.17g, hi = %.17g, bins = %d are not finite and strictly ascending",
                    lo, hi, bins);
    return SLICER_OK;
}

int slicer_peaks_create(slicer_handle h, int32_t npix, int32_t n_edges, const double *edges, slicer_peaks_handle *out)
{
    hipStream_t st = nullptr;
    slicer_peaks_handle ph = nullptr;
    int rc = rank_create(h, kPeaks, npix, n_edges, edges, out, &st, &ph);
    if (!ph)
        return rc;
    ph->B = n_edges - 1;
    // the LDS of a workgroup: the window, the edges, the counters
    ph->gmax = resident_groups(kRows * kPitch * sizeof(float) + peaks_dyn_lds(ph->B), tiles_of(npix), h->num_cus);
    const size_t nC = 3 * (size_t)ph->B + kOutside;
    rc = ph->mem.alloc(rc, h, kPeaks.create, (void **)&ph->partial, (size_t)ph->gmax * nC * sizeof(unsigned));
    rc = ph->mem.alloc(rc, h, kPeaks.create, (void **)&ph->res, nC * sizeof(int64_t));
    return sub_done(rank_upload(rc, *ph, kPeaks, st), ph, out);
}

int slicer_peaks_run_npix(slicer_peaks_handle ph, const float *d_map, int32_t npix)
{
    hipStream_t st;
    if (int rc = rank_run_begin(ph, d_map, npix, kPeaks, &st))
        return rc;
    const int nC = 3 * ph->B + kOutside;
    PeakArgs a{};
    a.x = d_map;
    a.edges = ph->d_table;
    a.partial = ph->partial;
    a.n = npix;
    a.B = ph->B;
    a.tiles_x = tiles_across(npix);
    a.ntiles = (int)tiles_of(npix);
    const int G = std::min(a.ntiles, ph->gmax);
    const size_t lds = peaks_dyn_lds(ph->B);
    {
        ProfScope ps(ph->h, KN_PEAKS);
        if (quads_aligned(d_map, npix))
            hipLaunchKernelGGL(k_peaks<true>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        else
            hipLaunchKernelGGL(k_peaks<false>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        HIPCHK(ph->h, hipGetLastError());
    }
    {
        ProfScope ps(ph->h, KN_PEAKS_FINISH);
        launch_column_sums(st, ph->partial, G, nC, ph->res);
        HIPCHK(ph->h, hipGetLastError());
    }
    ph->ran = true;
    return SLICER_OK;
}

int slicer_peaks_run(slicer_peaks_handle ph, const float *d_map)
{
    if (int rc = rank_not_null(ph, d_map, kPeaks, ""))
        return rc;
    return slicer_peaks_run_npix(ph, d_map, ph->n);
}

int slicer_peaks_read(slicer_peaks_handle ph, int64_t *pdf, int64_t *peaks, int64_t *minima, int64_t *below,
                      int64_t *above, int64_t *n_nan)
{
    if (int rc = rank_read_begin(ph, kPeaks))
        return rc;
    const size_t B = (size_t)ph->B;
    return read_slices(*ph, ph->res, {{pdf, B}, {peaks, B}, {minima, B}, {below, 3}, {above, 3}, {n_nan, 1}});
}

int slicer_peaks_destroy(slicer_peaks_handle ph) { return sub_destroy(ph); }

}  // extern "C"
