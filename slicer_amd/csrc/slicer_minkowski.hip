// slicer_minkowski.hip -- on-device Minkowski functionals of a map's excursion sets as exact counts.
//
// Of an n x n f32 map x (row-major, only read) and f64 thresholds t_0 < ... < t_{T-1}:
//   k(x)        the number of t_j <= (double)x, compared in f64 against the f64 thresholds; k(NaN) = k(-inf) = 0,
//               k(+inf) = T.  Pixel x is in the excursion set Q_j iff k(x) > j; positions outside the map have k = 0.
//   The map is a complex of n^2 closed unit squares (faces), 2 n (n + 1) unit edges and (n + 1)^2 vertices that does
//   not wrap; an edge or a vertex is in the closure of Q_j iff one of its adjacent faces is.  Per threshold j:
//   faces[j]    pixels with k > j                       vertices[j]  vertices with max k over their faces > j
//   edges[j]    edges with max k over their faces > j   border[j]    edges on the map's rim whose one face has k > j
//   boundary[j] interior edges with exactly one of their two faces in Q_j = #{max k > j} - #{min k > j}
//   n_nan       NaN pixels (in no set).
// Every count is an integer: nothing here is a floating-point sum, so the results are exact and the same on every run.
//
// k_minkowski works on the grid of (n + 1)^2 cells.  Cell (i, j), 0 <= i, j <= n, owns face (i, j), the vertex at its
// top-left corner, its top edge (between faces (i-1, j) and (i, j)) and its left edge (between faces (i, j-1) and
// (i, j)): every face, edge and vertex has exactly one owner, and an owned edge is on the rim iff i is 0 or n (top
// edge) or j is 0 or n (left edge).  What does not exist (a face or a left edge of row n, a top edge of column n,
// anything past them) has only faces of rank 0 and is never counted, so existence needs no test.
// The tile, the search, the four-pixel load, the counters' copies, the grid size, the column sums and the host side of
// the entry points are those of slicer_rank_counts.hpp.
// A workgroup of 256 threads takes tiles of kT0 x kT1 = 16 x 64 cells and every thread
// four adjacent cells of one row.  A tile needs the RANKS of 17 x 65 pixels: its own faces, one row above and one
// column to the left.  Every pixel of the window is searched once, while it is staged, and the window holds the ranks
// as u16 (k <= 1025), not the floats: 17 rows of pitch 72 with the tile's first column at window column 4, so that a
// thread's four ranks of a row are one 8-byte LDS access and the left neighbour one u16.  Thread t stages the four
// pixels of quad t % 16 of window row t / 16 (rows r0 - 1 ... r0 + 14) and, for t < 81, one more pixel: the tile's
// last row (t < 64) or the column to the left (64 <= t < 81).  The five are searched side by side in ONE pass of
// rank_search (ceil(log2 T) + 1 LDS reads of the f64 thresholds), so the 81 extra pixels cost a fifth more reads and no
// second pass.  Loads: a float4 per quad when 4 | n and
// the map is on the 16-byte grid (k_minkowski<true>), scalar loads otherwise (<false>); the window, and so the counts,
// are the same.  NaN pixels are counted where they are staged as one of the tile's own faces.
// Counters: five u32 LDS histograms of T + 1 rank bins -- face k, vertex max k, interior-edge max k, interior-edge
// min k, rim-edge k -- and the NaN counter, incremented with LDS integer atomics; rank 0 is in no set and is skipped.
// Lanes that hit one counter at once are served one after the other, and on a smooth map or with few thresholds most
// lanes of a wave do.  Two measures, neither changes a count: (1) the counters are kept in 2^c copies, c the largest
// with 2^c <= 32 and 2^c * 20 (T + 1) B <= 16 KB (32 copies at T = 9, 8 at 65, 1 above 408), copy `lane mod 2^c` of
// counter m at word m * 2^c + copy, so the copies of one counter lie in adjacent banks; the flush adds them.  (2) A
// thread whose ten ranks are equal (its four cells lie inside a plateau of rank r; rank 0 outside the map makes that
// impossible on the rim) adds 4 faces, 4 vertices and 8 interior edges (max and min) of rank r with four atomics
// instead of twenty-four.
// u32 is enough: the interior-edge histograms take at most 2 * 1024 increments a tile, a workgroup takes at most
// ceil(tiles / G) tiles, tiles <= 8193 * 2049 and G >= min(tiles, 64) (a static_assert).
// The grid is fixed: G = min(tiles, max(kMinGroups, w * CUs)) workgroups, w = min(8, what a CU's LDS holds at once),
// workgroup b takes tiles b, b + G, ...  Flush: workgroup b stores its counters as row b of partial[G][5 (T + 1) + 1];
// k_column_sums sums the rows of every column into int64, k_minkowski_suffix (one workgroup) forms
// out[j] = sum over k > j of hist[k] and stores faces, edges = edge max + rim, vertices, boundary = edge max - edge
// min, border = rim, and the NaN count.  Every row and every result is stored by every launch: nothing is zeroed
// between runs, nothing carried over, no global atomics.
#include <hip/hip_runtime.h>

#include "slicer_rank_counts.hpp"

namespace {

constexpr int kRows = kT0 + 1;       // window rows: one above the tile
constexpr int kExtra = kT1 + kRows;  // the tile's last row and the column to its left: one pixel a thread
constexpr int kMaxT = SLICER_MINKOWSKI_MAX_THRESHOLDS;
constexpr int kHists = 5;  // face, vertex, interior-edge max, interior-edge min, rim edge
enum { H_FACE = 0, H_VERTEX, H_EDGE_MAX, H_EDGE_MIN, H_RIM };
constexpr size_t kCopyBytes = 16 * 1024;  // LDS for the copies of the counters (one copy may be larger)

static_assert(kExtra <= kThreads && kQuads * (kRows - 1) == kThreads, "a quad and at most one more pixel a thread");
static_assert((((int64_t)kMaxNpix + 1 + kT0 - 1) / kT0) * (((int64_t)kMaxNpix + 1 + kT1 - 1) / kT1) / kMinGroups + 1 <
                  ((int64_t)1 << 32) / (2 * kT0 * kT1),
              "a workgroup's u32 counters hold the 2 * 1024 increments a tile of every tile it can meet");

struct MinkArgs {
    const float *x;
    const double *thr;  // [T]
    unsigned *partial;  // [gridDim.x][5 (T + 1) + 1]
    int n, T;
    int tiles_x, ntiles;
    int lg_copies;  // log2 of the copies of every counter in LDS
};

// log2 of the copies of the 5 (T + 1) counters that kCopyBytes hold, 32 at most
int lg_copies_of(int T) { return lg_copies((size_t)kHists * (T + 1) * sizeof(unsigned), kCopyBytes, 5); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_minkowski(MinkArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short win[kRows * kPitch];
    extern __shared__ double dyn[];
    const int n = a.n, T = a.T, nb = T + 1, nC = kHists * nb + 1, tid = threadIdx.x;
    const int lg = a.lg_copies, nan_at = (kHists * nb) << lg;  // counter (h, k), copy c: cnt[((h nb + k) << lg) + c]
    const unsigned copy = tid & ((1 << lg) - 1);
    double *thr = dyn;
    unsigned *cnt = reinterpret_cast<unsigned *>(dyn + T);
    stage_table<kThreads>(thr, a.thr, T);
    for (int k = tid; k <= nan_at; k += kThreads)
        cnt[k] = 0u;
    // w more elements of rank k in histogram h; rank 0 is in no set
    const auto add = [&](int h, unsigned k, unsigned w) {
        if (k)
            atomicAdd(&cnt[(((unsigned)(h * nb) + k) << lg) + copy], w);
    };
    const int lr = tid / kQuads, lc = tid % kQuads * kPer;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int r0 = t / a.tiles_x * kT0, c0 = t % a.tiles_x * kT1;
        __syncthreads();  // the previous tile's window has been read (first tile: thresholds and counters are in place)
        // the five pixels of this thread: v[0..3] the quad of window row lr (map row r0 - 1 + lr), v[4] the extra one.
        // A position outside the map stays -inf: rank 0, like the NaNs, which are counted here.
        float v[kPer + 1];
        {
            // (VEC: 4 | n and c % 4 == 0, so a quad lies in the map whole or not at all)
            const int r = r0 - 1 + lr, c = c0 + lc, have = r >= 0 && r < n && c < n ? (VEC ? kPer : min(n - c, kPer)) : 0;
            const float4 m = load_quad<VEC>(a.x, (size_t)r * n + c, have, -INFINITY);
            v[0] = m.x, v[1] = m.y, v[2] = m.z, v[3] = m.w, v[kPer] = -INFINITY;
        }
        int er = -1, ec = -1;  // the extra pixel's map position
        if (tid < kT1)
            er = r0 + kT0 - 1, ec = c0 + tid;
        else if (tid < kExtra)
            er = r0 - 1 + (tid - kT1), ec = c0 - 1;
        if (er >= 0 && er < n && ec >= 0 && ec < n)
            v[kPer] = a.x[(size_t)er * n + ec];
        unsigned n_nan = 0;  // among the tile's own faces: every row of the quads but the first, and the last row
#pragma unroll
        for (int q = 0; q < kPer; q++)
            n_nan += lr >= 1 && v[q] != v[q] ? 1u : 0u;
        n_nan += tid < kT1 && v[kPer] != v[kPer] ? 1u : 0u;
        if (n_nan)
            atomicAdd(&cnt[nan_at], n_nan);
        // pos[q]: how many of t_0 ... t_{T-1} are <= pixel q, the five side by side; a NaN has rank 0
        double xd[kPer + 1];
        int pos[kPer + 1];
#pragma unroll
        for (int q = 0; q <= kPer; q++)
            xd[q] = (double)v[q];
        rank_search(thr, T, xd, pos);
        *reinterpret_cast<uint2 *>(win + lr * kPitch + kLeft + lc) =
            make_uint2((unsigned)pos[0] | (unsigned)pos[1] << 16, (unsigned)pos[2] | (unsigned)pos[3] << 16);
        if (tid < kT1)
            win[(kRows - 1) * kPitch + kLeft + tid] = (unsigned short)pos[kPer];
        else if (tid < kExtra)
            win[(tid - kT1) * kPitch + kLeft - 1] = (unsigned short)pos[kPer];
        __syncthreads();
        const int i = r0 + lr, j0 = c0 + lc;
        if (i > n || j0 > n)
            continue;  // (only faces of rank 0 around these cells)
        // up[q], at[q]: the ranks of faces (i-1, j0-1+q) and (i, j0-1+q), q = 0 ... 4
        unsigned up[kPer + 1], at[kPer + 1];
        {
            const unsigned short *w = win + lr * kPitch + kLeft + lc;
            const uint2 u = *reinterpret_cast<const uint2 *>(w), d = *reinterpret_cast<const uint2 *>(w + kPitch);
            up[0] = w[-1], at[0] = w[kPitch - 1];
            up[1] = u.x & 0xffffu, up[2] = u.x >> 16, up[3] = u.y & 0xffffu, up[4] = u.y >> 16;
            at[1] = d.x & 0xffffu, at[2] = d.x >> 16, at[3] = d.y & 0xffffu, at[4] = d.y >> 16;
        }
        // Ten equal ranks: none of the ten faces is outside the map (rank 0 counts nothing), so the four cells' faces,
        // vertices and eight edges are all inside, all of that rank: four increments instead of twenty-four
        bool flat = true;
#pragma unroll
        for (int q = 0; q <= kPer; q++)
            flat = flat && up[q] == at[1] && at[q] == at[1];
        if (flat) {
            add(H_FACE, at[1], kPer);
            add(H_VERTEX, at[1], kPer);
            add(H_EDGE_MAX, at[1], 2 * kPer);
            add(H_EDGE_MIN, at[1], 2 * kPer);
            continue;
        }
        const bool rim_row = i == 0 || i == n;
#pragma unroll
        for (int q = 0; q < kPer; q++) {
            const int j = j0 + q;
            const unsigned f = at[q + 1], left = at[q], above = up[q + 1];
            add(H_FACE, f, 1);
            add(H_VERTEX, max(max(up[q], above), max(left, f)), 1);
            if (rim_row) {  // the top edge: one of its two faces is outside
                add(H_RIM, max(above, f), 1);
            } else {
                add(H_EDGE_MAX, max(above, f), 1);
                add(H_EDGE_MIN, min(above, f), 1);
            }
            if (j == 0 || j == n) {  // the left edge
                add(H_RIM, max(left, f), 1);
            } else {
                add(H_EDGE_MAX, max(left, f), 1);
                add(H_EDGE_MIN, min(left, f), 1);
            }
        }
    }
    __syncthreads();
    unsigned *out = a.partial + (size_t)blockIdx.x * nC;
    for (int k = tid; k < nC - 1; k += kThreads)
        out[k] = fold_copies(cnt, k, lg);
    if (tid == 0)
        out[nC - 1] = cnt[nan_at];
}

// One workgroup: suf[h][k] = sum over m >= k of histogram h.  Thread u sums the bins u per ... (u + 1) per - 1 of every
// histogram, the 256 chunk sums are scanned from the back in eight doubling steps, and every thread walks its bins down
// from the sum of the chunks after its own.  Then res = faces [T], edges [T], vertices [T], boundary [T], border [T],
// n_nan with out[j] = suf[j + 1].
__global__ __launch_bounds__(kThreads) void k_minkowski_suffix(const int64_t *hist, int T, int64_t *res)
{
    __shared__ int64_t suf[kHists][kMaxT + 1];
    __shared__ int64_t chunk[kHists][kThreads];
    const int nb = T + 1, tid = threadIdx.x, per = (nb + kThreads - 1) / kThreads;
    const int lo = min(tid * per, nb), hi = min(lo + per, nb);
    int64_t own[kHists];
    for (int h = 0; h < kHists; h++) {
        own[h] = 0;
        for (int k = lo; k < hi; k++)
            own[h] += hist[(size_t)h * nb + k];
        chunk[h][tid] = own[h];
    }
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        int64_t more[kHists];
        for (int h = 0; h < kHists; h++)
            more[h] = tid + off < kThreads ? chunk[h][tid + off] : 0;
        __syncthreads();
        for (int h = 0; h < kHists; h++)
            chunk[h][tid] += more[h];
        __syncthreads();
    }
    for (int h = 0; h < kHists; h++) {
        int64_t run = chunk[h][tid] - own[h];  // the chunks after this thread's
        for (int k = hi - 1; k >= lo; k--) {
            run += hist[(size_t)h * nb + k];
            suf[h][k] = run;
        }
    }
    __syncthreads();
    for (int j = tid; j < T; j += kThreads) {
        const int64_t edge_max = suf[H_EDGE_MAX][j + 1], rim = suf[H_RIM][j + 1];
        res[j] = suf[H_FACE][j + 1];
        res[T + j] = edge_max + rim;
        res[2 * T + j] = suf[H_VERTEX][j + 1];
        res[3 * T + j] = edge_max - suf[H_EDGE_MIN][j + 1];
        res[4 * T + j] = rim;
    }
    if (tid == 0)
        res[5 * T] = hist[kHists * nb];
}

size_t mink_columns(int T) { return (size_t)kHists * ((size_t)T + 1) + 1; }

// the thresholds, the copies of the 5 (T + 1) counters and the NaN counter
size_t mink_dyn_lds(int T)
{
    return (size_t)T * sizeof(double) + (((mink_columns(T) - 1) << lg_copies_of(T)) + 1) * sizeof(unsigned);
}

const RankModule kMinkowski = {"slicer_minkowski", "slicer_minkowski_create", "thresholds", "fewer than 1 threshold", 1, kMaxT,
                               kMaxNpix};

}  // namespace

struct slicer_minkowski : RankHandle {  // table: the T thresholds
    int T = 0;
    unsigned *partial = nullptr;
    int64_t *hist = nullptr;  // the column sums of `partial`
    int64_t *res = nullptr;
};

extern "C" {

int slicer_minkowski_create(slicer_handle h, int32_t npix, int32_t n_thresholds, const double *thresholds,
                            slicer_minkowski_handle *out)
{
    hipStream_t st = nullptr;
    slicer_minkowski_handle mh = nullptr;
    int rc = rank_create(h, kMinkowski, npix, n_thresholds, thresholds, out, &st, &mh);
    if (!mh)
        return rc;
    mh->T = n_thresholds;
    // the LDS of a workgroup: the window, the thresholds, the counters; the tiles cover the n + 1 cells of a side
    mh->gmax = resident_groups(kRows * kPitch * sizeof(unsigned short) + mink_dyn_lds(mh->T), tiles_of(npix + 1), h->num_cus);
    const size_t nC = mink_columns(mh->T);
    rc = mh->mem.alloc(rc, h, kMinkowski.create, (void **)&mh->partial, (size_t)mh->gmax * nC * sizeof(unsigned));
    rc = mh->mem.alloc(rc, h, kMinkowski.create, (void **)&mh->hist, nC * sizeof(int64_t));
    rc = mh->mem.alloc(rc, h, kMinkowski.create, (void **)&mh->res, (5 * (size_t)mh->T + 1) * sizeof(int64_t));
    return sub_done(rank_upload(rc, *mh, kMinkowski, st), mh, out);
}

int slicer_minkowski_run_npix(slicer_minkowski_handle mh, const float *d_map, int32_t npix)
{
    hipStream_t st;
    if (int rc = rank_run_begin(mh, d_map, npix, kMinkowski, &st))
        return rc;
    const int nC = (int)mink_columns(mh->T);
    MinkArgs a{};
    a.x = d_map;
    a.thr = mh->d_table;
    a.partial = mh->partial;
    a.n = npix;
    a.T = mh->T;
    a.tiles_x = tiles_across(npix + 1);
    a.ntiles = (int)tiles_of(npix + 1);
    a.lg_copies = lg_copies_of(mh->T);
    const int G = std::min(a.ntiles, mh->gmax);
    const size_t lds = mink_dyn_lds(mh->T);
    {
        ProfScope ps(mh->h, KN_MINKOWSKI);
        if (quads_aligned(d_map, npix))
            hipLaunchKernelGGL(k_minkowski<true>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        else
            hipLaunchKernelGGL(k_minkowski<false>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        HIPCHK(mh->h, hipGetLastError());
    }
    {
        ProfScope ps(mh->h, KN_MINKOWSKI_FINISH);
        launch_column_sums(st, mh->partial, G, nC, mh->hist);
        HIPCHK(mh->h, hipGetLastError());
        hipLaunchKernelGGL(k_minkowski_suffix, dim3(1), dim3(kThreads), 0, st, mh->hist, mh->T, mh->res);
        HIPCHK(mh->h, hipGetLastError());
    }
    mh->ran = true;
    return SLICER_OK;
}

int slicer_minkowski_run(slicer_minkowski_handle mh, const float *d_map)
{
    if (int rc = rank_not_null(mh, d_map, kMinkowski, ""))
        return rc;
    return slicer_minkowski_run_npix(mh, d_map, mh->n);
}

int slicer_minkowski_read(slicer_minkowski_handle mh, int64_t *faces, int64_t *edges, int64_t *vertices, int64_t *boundary,
                          int64_t *border, int64_t *n_nan)
{
    if (int rc = rank_read_begin(mh, kMinkowski))
        return rc;
    const size_t T = (size_t)mh->T;
    return read_slices(*mh, mh->res, {{faces, T}, {edges, T}, {vertices, T}, {boundary, T}, {border, T}, {n_nan, 1}});
}

int slicer_minkowski_destroy(slicer_minkowski_handle mh) { return sub_destroy(mh); }

}  // extern "C"
