// slicer_binned_common.hpp -- SLICER_ALGO_BINNED: project -> per-tile bins -> LDS-privatised tile deposit.  The overview
// of the path, and what its kernels share (slicer_project_bin.hip: K1; slicer_sort.hip: K2, K3; slicer_tile_deposit.hip:
// K4).  gfx950 only.
//
// Why: a TSC deposit is 9 read-modify-writes on a random pixel; as global float atomics that is
// ~0.08 TB/s of added bytes on MI355X (64 lanes in 64 rows; MI355X_MICROARCH.md "Global float
// atomics"), i.e. ~2e9 particles/s.  Here the scatter is done in LDS instead:
//
//   K1 k_project_bin_* : (slicer_project_bin.hip) stream raw POS (12 B/particle, dwordx4 loads), bit-faithful
//                        transform, slab select, fp64 projection; emits (xs, ys) records + their tile bin, a
//                        per-workgroup histogram row and the workgroup's record counts.  No global atomics on the
//                        data path.
//   K2 k_scan_blocks   : exclusive prefix over (bin-major, workgroup-minor) -> every K1 workgroup's write cursor for
//                        every bin (radix-partition style; no atomics), plus in-group bin prefixes and group sums
//                        from which K3 derives the bin bases itself.
//   K3 k_bin_scatter   : moves each record to its bin's contiguous run: persistent workgroups counting-sort
//                        the records of one (plane, K1 workgroup) region by tile in LDS and store them in
//                        tile order (coalesced runs).
//   K4 k_tile_deposit  : one workgroup per (plane, tile) (more for heavy tiles): tile + 1-pixel halo
//                        privatised in LDS as 8-byte cells (f64 or integer) or 4-byte NGP counts, one software-pipelined
//                        walk over all pending chunks, then one shaped (row-contiguous) flush of the non-zero cells;
//                        NGP counts of whole sub-files are folded into the f32 maps at the file boundaries of the walk.
//
// Replaces the CPU loops of gadget2io.cpp:195-274, densitymaps.cpp:355-401 and utilities.cpp:66-95.
#pragma once
#include <type_traits>
#include <utility>

#include "slicer_kernels.hpp"

namespace slicer {

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

template <typename T>
__device__ __forceinline__ T dmin(T a, T b) { return a < b ? a : b; }

#ifndef SLICER_LDS_BARRIER
#define SLICER_LDS_BARRIER 1
#endif
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the global-memory queue
// (s_waitcnt vmcnt(0)), which stalls every wave on loads and stores that nothing behind the barrier depends on.
// Use where the barrier protects LDS contents; register dependences on loaded values are tracked by the compiler.
__device__ __forceinline__ void lds_barrier()
{
#if SLICER_LDS_BARRIER
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#else
    __syncthreads();
#endif
}

// LDS traffic of this wave is complete and the compiler may not move memory operations across
__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Sorted record of the per-particle-mass (hydro) path: (xs, ys, m) in one 12-byte store / load.  The constant-mass path
// keeps 8-byte float2 records; PendingList::sxy points at one or the other (sm != nullptr tells which).
struct __attribute__((packed, aligned(4))) Rec3 {
    float x, y, m;
};

// (unit, tile-in-unit) of a map cell under the tile geometry G.  A unit is a plane, or a band of rows_per_unit tile
// rows of a plane on large maps (BinGeom).
__device__ __forceinline__ void cell_to_tile(int gx, int gy, int plane, const BinGeom &G, unsigned &unit,
                                             unsigned &tile_in_unit)
{
    const unsigned ty = (unsigned)(gy >> G.th_log2), tx = (unsigned)(gx >> G.tw_log2);
    unsigned band = 0, trow = ty;
    if (G.units_per_plane > 1) {
        band = ty / (unsigned)G.rows_per_unit;
        trow = ty - band * (unsigned)G.rows_per_unit;
    }
    unit = (unsigned)plane * (unsigned)G.units_per_plane + band;
    tile_in_unit = trow * (unsigned)G.ntx + tx;
}

// Launch `kern` with `lds` bytes of dynamic LDS.  A kernel gets 48 KiB without asking; its limit is raised first where
// `lds` exceeds `raise_above` (0: always).
template <typename... Params, typename... Args>
inline hipError_t launch_with_lds(void (*kern)(Params...), unsigned grid, unsigned block, size_t lds, size_t raise_above,
                                  hipStream_t s, Args &&...args)
{
    if (lds > raise_above) {
        const hipError_t e =
            hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return e;
    }
    kern<<<grid, block, lds, s>>>(std::forward<Args>(args)...);
    return hipGetLastError();
}

}  // namespace slicer
