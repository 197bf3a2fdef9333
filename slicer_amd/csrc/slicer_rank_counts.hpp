// slicer_rank_counts.hpp -- internal: what slicer_peaks.hip and slicer_minkowski.hip (row N14) share,
// device and host; slicer_starlet.hip (row N16) takes the search, the column sums and the host helpers for its binned
// sums, and slicer_betti.hip (row N19) the same.  Only those four include it; everything is in an unnamed namespace, so each has its own copy (the column-sum
// kernel too: kernels of one name, one per code object).
// Both count integers over tiles of kT0 x kT1 = 16 x 64 positions (the tile of slicer_fd.hip), four adjacent ones of a
// row a thread, from a window in LDS whose rows have pitch 72 with the tile's first column at window column 4, so that
// the quads of a row sit on LDS's 16-byte grid.  Both rank a pixel among ascending f64 values in LDS (rank_search), keep
// u32 counters in LDS, store them as one row of partial[G][nC] a workgroup, and k_column_sums adds the rows in int64.
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

// Workgroup v sums columns 16 v ... 16 v + 15 of partial[G][nC] into sums[nC]: sixteen threads a column, thread rg of
// them the rows rg, rg + 16, ...; integer sums, so the order does not matter.
__global__ __launch_bounds__(kThreads) void k_column_sums(const unsigned *partial, int G, int nC, int64_t *sums)
{
    __shared__ int64_t red[kFinRows][kFinCols];
    const int cl = threadIdx.x % kFinCols, rg = threadIdx.x / kFinCols, col = (int)blockIdx.x * kFinCols + cl;
    int64_t acc = 0;
    if (col < nC) {
#pragma unroll 8
        for (int g = rg; g < G; g += kFinRows)
            acc += (int64_t)partial[(size_t)g * nC + col];
    }
    red[rg][cl] = acc;
    __syncthreads();
    if (rg != 0 || col >= nC)
        return;
    for (int k = 1; k < kFinRows; k++)
        acc += red[k][cl];
    sums[col] = acc;
}

void launch_column_sums(hipStream_t st, const unsigned *partial, int G, int nC, int64_t *sums)
{
    hipLaunchKernelGGL(k_column_sums, dim3((unsigned)((nC + kFinCols - 1) / kFinCols)), dim3(kThreads), 0, st, partial, G,
                       nC, sums);
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
