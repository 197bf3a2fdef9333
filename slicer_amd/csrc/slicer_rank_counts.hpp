// slicer_rank_counts.hpp -- internal: the core of the four map statistics that rank every pixel of an f32 map against an
// ascending f64 table (edges or thresholds) held in LDS, count into u32 LDS counters, store one row of partials a
// workgroup and sum the rows in a small finish kernel.  Four files include it: slicer_peaks.hip,
// slicer_minkowski.hip (row N14), slicer_starlet.hip for its l1-norm (row N16) and slicer_betti.hip (row N19).
// Everything is in an unnamed namespace, so each has its own copy (the column-sum kernels too: kernels of one name, one
// per code object).
// Device: the tile of kT0 x kT1 = 16 x 64 positions (the tile of slicer_fd.hip), four adjacent ones of a row a thread,
// whose LDS window has rows of pitch 72 with the tile's first column at window column 4, so that the quads of a row
// sit on LDS's 16-byte grid (peaks, Minkowski); the table's way into LDS (stage_table) and the search in it
// (rank_search); the four-pixel load (load_quad); a pixel's bin by the PDF rule (pdf_slot); counters kept in 2^lg
// striped copies (lg_copies on the host, fold_copies at the flush); and k_column_sums, which adds the rows of
// partial[G][nC].
// Host: RankHandle, the base of the four handle structs, and what their entry points share, told apart by a RankModule
// of names and limits: rank_create and rank_upload for a *_create, rank_run_begin for a *_run_npix, rank_not_null for a
// *_run, rank_read_begin and read_slices for a *_read.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <utility>
#include <vector>

#include "slicer_host.hpp"

namespace {

constexpr int kT0 = 16, kT1 = 64;  // tile: rows x columns
constexpr int kPer = 4;            // adjacent positions of a thread
constexpr int kThreads = kT0 * kT1 / kPer;
constexpr int kLeft = 4;                 // window column of the tile's first pixel
constexpr int kPitch = kLeft + kT1 + 4;  // 72 elements: every window row starts on the 16-byte grid
constexpr int kQuads = kT1 / kPer;       // quads of a tile row = threads of a tile row
constexpr int kMaxNpix = 131072;
constexpr int kPerCu = 8, kMinGroups = 64;   // workgroups per CU at most; fewer where their LDS does not fit
constexpr int kFinCols = 16, kFinRows = 16;  // k_column_sums: columns of a workgroup x threads of a column

static_assert(kThreads == 256 && kFinCols * kFinRows == kThreads, "one thread per four positions of a tile");

// table[0 .. len-1] into LDS by the THREADS threads of a workgroup (no barrier: the caller's)
template <int THREADS>
__device__ __forceinline__ void stage_table(double *lds, const double *table, int len)
{
    for (int k = threadIdx.x; k < len; k += THREADS)
        lds[k] = table[k];
}

// pos[q]: how many of table[0 .. len-1] (ascending) are <= x[q].  Invariant of the search: every entry before `pos` is
// <= x and the answer lies in pos ... pos + len.  The steps depend on len alone, so the wave never diverges, and the N
// pixels' reads of a step are independent of one another: ceil(log2 len) + 1 reads a pixel -- the rule itself, no guess
// to correct.  A NaN fails every comparison: 0.
template <int N>
__device__ __forceinline__ void rank_search(const double *table, int len, const double (&x)[N], int (&pos)[N])
{
#pragma unroll
    for (int q = 0; q < N; q++)
        pos[q] = 0;
    while (len > 1) {
        const int half = len / 2;
#pragma unroll
        for (int q = 0; q < N; q++)
            pos[q] = table[pos[q] + half - 1] <= x[q] ? pos[q] + half : pos[q];
        len -= half;
    }
#pragma unroll
    for (int q = 0; q < N; q++)
        pos[q] += table[pos[q]] <= x[q] ? 1 : 0;
}

// The PDF rule (numpy.histogram's, N10): of a pixel x with pos of the edges e_0 ... e_{B-1} <= x, the bin pos - 1 --
// e_{B-1} <= x <= e_B gives pos = B: the last bin is closed -- or, in the caller's layout of its counters, `outside`:
// below e_0, outside + step: above e_B, outside + 2 step: NaN.
__device__ __forceinline__ int pdf_slot(double x, int pos, double eB, int outside, int step)
{
    if (x != x)
        return outside + 2 * step;
    if (pos == 0)
        return outside;
    return x > eB ? outside + step : pos - 1;
}

// The pixels first ... first + 3 of x, the last 4 - have of them (outside the map) as `fill`: a float4 when x + first is on
// the 16-byte grid (VEC) and the quad is whole, scalar loads otherwise.
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float *x, size_t first, int have, float fill)
{
    if (VEC && have == kPer)
        return *reinterpret_cast<const float4 *>(x + first);
    float v[kPer];
#pragma unroll
    for (int e = 0; e < kPer; e++) {
        v[e] = fill;
        if (e < have)
            v[e] = x[first + e];
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// Counters in LDS are kept in 2^lg copies so that lanes that hit one counter at once are not served one after the other:
// a thread adds into copy `thread mod 2^lg` of counter k at cnt[(k << lg) + copy], the copies of one counter in adjacent
// banks.  lg_copies: the largest lg <= lg_max whose copies of copy_bytes each fit the budget (one copy may be larger).
int lg_copies(size_t copy_bytes, size_t budget, int lg_max)
{
    int lg = 0;
    while (lg < lg_max && (copy_bytes << (lg + 1)) <= budget)
        lg++;
    return lg;
}

// ... and the flush: the copies of counter k, added in index order from copy 0 on (f64 sums depend on it).
template <class T>
__device__ __forceinline__ T fold_copies(const T *cnt, int k, int lg)
{
    T sum = cnt[(size_t)k << lg];
    for (int c = 1; c < 1 << lg; c++)
        sum = sum + cnt[((size_t)k << lg) + c];
    return sum;
}

// Workgroup v sums columns 16 v ... 16 v + 15 of partial[G][nC] into sums[nC]: sixteen threads a column, thread rg of
// them the rows rg, rg + 16, ... in that order, then thread 0 of them the sixteen in order.  <unsigned, int64_t> for the
// counts, where the order does not matter; <double, double> for f64 sums, whose order this fixes (no fast-math, no
// contraction: unrolling does not reassociate).
template <class TIn, class TAcc>
__global__ __launch_bounds__(kThreads) void k_column_sums(const TIn *partial, int G, int nC, TAcc *sums)
{
    __shared__ TAcc red[kFinRows][kFinCols];
    const int cl = threadIdx.x % kFinCols, rg = threadIdx.x / kFinCols, col = (int)blockIdx.x * kFinCols + cl;
    TAcc acc = 0;
    if (col < nC) {
#pragma unroll 8
        for (int g = rg; g < G; g += kFinRows)
            acc = acc + (TAcc)partial[(size_t)g * nC + col];
    }
    red[rg][cl] = acc;
    __syncthreads();
    if (rg != 0 || col >= nC)
        return;
    for (int k = 1; k < kFinRows; k++)
        acc = acc + red[k][cl];
    sums[col] = acc;
}

template <class TIn, class TAcc>
void launch_column_sums(hipStream_t st, const TIn *partial, int G, int nC, TAcc *sums)
{
    hipLaunchKernelGGL((k_column_sums<TIn, TAcc>), dim3((unsigned)((nC + kFinCols - 1) / kFinCols)), dim3(kThreads), 0, st,
                       partial, G, nC, sums);
}

int tiles_across(int cells) { return (cells + kT1 - 1) / kT1; }
int64_t tiles_of(int cells) { return (int64_t)((cells + kT0 - 1) / kT0) * tiles_across(cells); }

// The fixed grid: as many workgroups as are resident at once -- by the LDS of one, kPerCu a CU at most -- but at least
// kMinGroups, and no more than there are tiles.
int resident_groups(size_t lds_bytes, int64_t tiles, int num_cus)
{
    constexpr size_t kLdsPerCu = 160 * 1024;  // gfx950
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(kPerCu, kLdsPerCu / lds_bytes));
    return (int)std::min<int64_t>(tiles, std::max(kMinGroups, per_cu * num_cus));
}

// the float4 path: 4 | npix and the map on the 16-byte grid, so a quad lies in the map whole or not at all
bool quads_aligned(const float *d_map, int npix) { return npix % 4 == 0 && (uintptr_t)d_map % 16 == 0; }

// 0, or what the values (edges, thresholds) must be and are not: "finite", "strictly ascending"
const char *ascending_fault(int32_t n, const double *v)
{
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k]))
            return "finite";
    for (int k = 1; k < n; k++)
        if (!(v[k - 1] < v[k]))
            return "strictly ascending";
    return nullptr;
}

// ---- host: what the four handles and their entry points share ----
struct RankHandle : SubHandle {
    int n = 0;                  // the largest map side
    int gmax = 0;               // rows of the partials
    std::vector<double> table;  // the edges or thresholds, and their device copy
    double *d_table = nullptr;
    bool ran = false;
};

// What tells the modules' entry points apart: their names (stem "slicer_peaks" for slicer_peaks_run ...), what the
// table's values are called, and the limits of a *_create.
struct RankModule {
    const char *stem, *create;
    const char *nouns, *too_few;  // "edges", "fewer than 2 edges"
    int min_count, max_count, max_npix;
};

// A *_create up to its own allocations.  The numbers first: they need no handle, so a caller can have them checked
// before any device exists.  Then sub_new, the base filled in and the table's device copy allocated.  *x stays null where
// the call was refused (the return value says why); otherwise the return value goes through the module's own mem.alloc
// calls and rank_upload into sub_done.
template <class T>
int rank_create(slicer_handle h, const RankModule &m, int32_t npix, int32_t count, const double *table, T **out,
                hipStream_t *st, T **x)
{
    *x = nullptr;
    if (out)
        *out = nullptr;
    if (int rc = npix_in_range(h, m.create, npix, m.max_npix))
        return rc;
    if (count < m.min_count)
        return fail(h, SLICER_ERR_ARG, "%s: %s", m.create, m.too_few);
    if (count > m.max_count)
        return fail(h, SLICER_ERR_ARG, "%s: %d %s, at most %d", m.create, count, m.nouns, m.max_count);
    if (!table)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", m.create);
    if (const char *what = ascending_fault(count, table))
        return fail(h, SLICER_ERR_ARG, "%s: %s must be %s", m.create, m.nouns, what);
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", m.create);
    if (int rc = sub_new(h, m.create, st, x))
        return rc;
    (*x)->n = npix;
    (*x)->table.assign(table, table + count);
    return (*x)->mem.alloc(SLICER_OK, h, m.create, (void **)&(*x)->d_table, (size_t)count * sizeof(double));
}

// ... and the table's upload after them (x.table outlives the copy); an earlier failure passes through.
int rank_upload(int rc, const RankHandle &x, const RankModule &m, hipStream_t st)
{
    if (rc != SLICER_OK)
        return rc;
    hipError_t e = hipMemcpyAsync(x.d_table, x.table.data(), x.table.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess)
        return fail(x.h, SLICER_ERR_HIP, "%s: copying the %s: %s", m.create, m.nouns, hipGetErrorString(e));
    return SLICER_OK;
}

// The refusal of a *_run<suffix> ("", "_npix") without a handle or a map
int rank_not_null(const RankHandle *x, const float *d_map, const RankModule &m, const char *suffix)
{
    if (!x || !d_map)
        return fail(x ? x->h : nullptr, SLICER_ERR_ARG, "%s_run%s: null argument", m.stem, suffix);
    return SLICER_OK;
}

// A *_run_npix before its launches: the refusals, the stream, and no results until the launches are enqueued.
int rank_run_begin(RankHandle *x, const float *d_map, int32_t npix, const RankModule &m, hipStream_t *st)
{
    if (int rc = rank_not_null(x, d_map, m, "_npix"))
        return rc;
    if (npix < 1 || npix > x->n)
        return fail(x->h, SLICER_ERR_ARG, "%s_run_npix: npix = %d outside 1..%d", m.stem, npix, x->n);
    if (int rc = sub_stream(x->h, x->device, st))
        return rc;
    x->ran = false;
    return SLICER_OK;
}

// A *_read before its copies
int rank_read_begin(const RankHandle *x, const RankModule &m)
{
    if (!x)
        return fail(nullptr, SLICER_ERR_ARG, "%s_read: null handle", m.stem);
    if (!x->ran)
        return fail(x->h, SLICER_ERR_STATE, "%s_read before any %s_run", m.stem, m.stem);
    return SLICER_OK;
}

// The results d_res, one run of int64 after the other, to the caller's arrays: {array or null, length} in their order.
int read_slices(const SubHandle &s, const int64_t *d_res, std::initializer_list<std::pair<int64_t *, size_t>> outs)
{
    size_t total = 0;
    for (const auto &o : outs)
        total += o.second;
    std::vector<int64_t> r(total);
    if (int rc = sub_read(s, r.data(), d_res, total * sizeof(int64_t)))
        return rc;
    size_t at = 0;
    for (const auto &o : outs) {
        if (o.first)
            std::copy_n(&r[at], o.second, o.first);
        at += o.second;
    }
    return SLICER_OK;
}

}  // namespace
