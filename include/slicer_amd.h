/*
 * slicer_amd.h -- C ABI of the MI355X-native particle->grid mass-assignment path.
 *
 * This is the drop-in boundary behind SLICER's createDensityMaps()
 * (reference: SLICER/densitymaps.h:161-165, body densitymaps.cpp:419-524, called
 * from slicer-v2.cpp:204-206).  The reference has no FFI; its seam is a C++ free
 * function over std::valarray / std::vector / ifstream.  The adapter in
 * slicer_amd/csrc/densitymaps_amd.{hpp,cpp} keeps that C++ signature and forwards
 * to the entry points below, which are what a binding for this path would bind:
 * plain pointers, sizes and PODs only -- no C++ types, no torch types.
 *
 * Call sequence for one lens plane (= one createDensityMaps call), per device:
 *
 *   slicer_create()                                  once per device
 *   slicer_plane_begin(desc)                         densitymaps.cpp:426-431  (resize/zero maps)
 *   for each snapshot sub-file ff in [ffmin,ffmax):  densitymaps.cpp:432
 *     slicer_file_begin(file)                        Header + Random entry    (:438, gadget2io.cpp:204-270)
 *     for each particle type t with npart[t] > 0:
 *       slicer_deposit_host|device(t, pos, mass, n)  readPos + mapParticles + gridist_w
 *     slicer_file_end()                              densitymaps.cpp:511-513  (per-file accumulation)
 *   slicer_plane_finalize()                          device maps final (ready for the cross-rank sum,
 *                                                    slicer-v2.cpp:214-217 -> RCCL, see slicer_amd_rccl.h)
 *   slicer_plane_read(...)                           D2H into the caller's valarrays; reports the
 *                                                    negativity guard of densitymaps.cpp:334-345
 *
 * All functions return 0 on success and a SLICER_ERR_* code otherwise; they never
 * exit(), abort() or throw across the boundary (the reference returns 1 and lets
 * main() MPI_Abort: slicer-v2.cpp:204-207; gridist_w calls exit(-1): utilities.cpp:55-64).
 * A handle is not thread-safe; different handles are independent (one per GPU).
 */
#ifndef SLICER_AMD_H
#define SLICER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLICER_AMD_VERSION 200 /* 0.2.0 */
#define SLICER_MAX_PLANES 8

/* status codes */
#define SLICER_OK 0
#define SLICER_ERR_NEGATIVE_COORD 1 /* densitymaps.cpp:334-345 "I will STOP here" -> reference returns 1 */
#define SLICER_ERR_ARG 2
#define SLICER_ERR_STATE 3
#define SLICER_ERR_HIP 4
#define SLICER_ERR_NOMEM 5
#define SLICER_ERR_UNSUPPORTED 6 /* e.g. SLICER_ALGO_BINNED asked for a pass it cannot serve */
#define SLICER_ERR_NO_DEVICE 7

/* mass-assignment scheme: DO_NGP is a compile-time macro in the reference (densitymaps.h:22),
 * a run-time argument of gridist_w (utilities.h:140) and a run-time field here. */
#define SLICER_MAS_TSC 0
#define SLICER_MAS_NGP 1

/* accumulator of the TSC maps (NGP always uses exact u32 counts when the mass is constant) */
#define SLICER_ACC_F32 0     /* f32 atomics: fastest, order-dependent in the last bits            */
#define SLICER_ACC_F64 1     /* f64 atomics, rounded to f32 once at finalize                       */
#define SLICER_ACC_FIXED64 2 /* 64-bit fixed point: order-independent => bitwise reproducible sums (also across ranks).
                              * ABSOLUTE accuracy: every contribution is rounded to 2^-fixed_frac_bits (default 2^-40) of
                              * the mass scale 2^ceil(log2 m) -- or of 2^10 (MAX_M) with per-particle masses -- so a pixel
                              * that holds nothing but a vanishing TSC weight (<< 1e-6 m) loses RELATIVE precision; pixels
                              * holding >= 1e-3 m agree with the f64 accumulator to < 1 f32 ulp.  F32 / F64 keep the
                              * relative per-pixel bound.  A cell overflows at 2^(64 - fixed_frac_bits) mass scales. */

/* deposit algorithm */
#define SLICER_ALGO_AUTO 0
#define SLICER_ALGO_DIRECT 1 /* fused project + global atomics                                   */
#define SLICER_ALGO_BINNED 2 /* project -> tile bins -> LDS-privatised tiles -> shaped row flush.  A pass with more
                             * (plane, tile) bins than one run holds, or with overlapping slabs, goes in plane groups;
                             * more than three lateral replications per side go in windows of the replica grid.
                             * An explicit BINNED request that cannot be honoured (a tile table beyond the limits) returns
                             * SLICER_ERR_UNSUPPORTED; only SLICER_ALGO_AUTO falls back to DIRECT
                             * (slicer_plane_algo_mask tells which ran). */

/* element kind of an accumulator map (slicer_plane_accumulators) */
#define SLICER_ELEM_F32 0
#define SLICER_ELEM_F64 1
#define SLICER_ELEM_FIXED64 2 /* u64, value = integer * 2^-fixed_exp */

typedef struct slicer_handle_s *slicer_handle;

/* One pass = up to SLICER_MAX_PLANES lens planes cut from the same box replication (same Random
 * entry and rcase: densitymaps.cpp:227-246, slicer-v2.cpp:184-185).  n_planes = 1 reproduces one
 * createDensityMaps call.  ld/ld2 are Lens.ld/ld2 in Mpc/h (data.h:111-112). */
typedef struct {
    int32_t npix;                          /* InputParams.npix (data.h:31)                       */
    int32_t n_planes;                      /* 1..SLICER_MAX_PLANES                               */
    int32_t mas;                           /* SLICER_MAS_*                                       */
    int32_t accum;                         /* SLICER_ACC_*  (TSC)                                */
    int32_t algo;                          /* SLICER_ALGO_*                                      */
    int32_t hydro;                         /* InputParams.hydro (data.h:35)                      */
    int32_t snopt;                         /* InputParams.snopt (data.h:45); > 0 draws libc rand(), plane-major */
    int32_t want_type_maps;                /* 1: keep the six per-type maps (mapxytoti)          */
    double fov_rad;                        /* fovradiants                                        */
    double ld[SLICER_MAX_PLANES];          /* Lens.ld[isnap]                                     */
    double ld2[SLICER_MAX_PLANES];         /* Lens.ld2[isnap]                                    */
    int32_t nrepperp[SLICER_MAX_PLANES];   /* Lens.nrepperp[isnap] (data.h:114)                  */
    int32_t fixed_frac_bits;               /* SLICER_ACC_FIXED64: fractional bits, 0 = auto (40) */
    int32_t debug_flags;                   /* bit 0: always use libm (OCML) asin/atan2, no small-angle series */
} slicer_plane_desc;

/* Per sub-file state: the fields of Header (data.h:59-79) and of the plane's Random entry
 * (data.h:126-131) that the path reads, plus rcase (slicer-v2.cpp:184-185). */
typedef struct {
    int32_t npart[6];   /* Header.npart                                  */
    double massarr[6];  /* Header.massarr                                */
    double boxsize;     /* Header.boxsize (kpc/h; POS_U = 1)             */
    int32_t sgn[3];     /* Random.sgnX/Y/Z[isnap]  (+1 / -1)             */
    int32_t face;       /* Random.face[isnap]      (1..6)                */
    double center[3];   /* Random.x0/y0/z0[isnap]                        */
    float rcase;        /* box-replication offset along the line of sight */
    int32_t reserved;
} slicer_file_desc;

typedef struct {
    char name[32];
    uint64_t launches;
    double total_ms; /* summed HIP-event time of those launches */
} slicer_kernel_time;

int slicer_version(void);

/* device = HIP device ordinal.  max_chunk = largest number of particles one deposit call may
 * carry in one kernel pass (bigger inputs are looped internally); sizes the workspace. */
int slicer_create(int device, uint64_t max_chunk, slicer_handle *out);
int slicer_destroy(slicer_handle h);
const char *slicer_last_error(slicer_handle h); /* valid until the next call on h; h may be NULL */

/* Tuning and test knobs of a handle (integers).  The environment seeds them once, in slicer_create (SLICER_<KEY> in
 * upper case); afterwards only this call changes them -- no launch path reads the environment, so handles driven by
 * different host threads (SLICER_amd --devices) do not share mutable state.  Not while deposits are in flight (an
 * open file, or chunks waiting for their tile launch: SLICER_ERR_STATE).  Keys:
 *   k4_int       integer (u64) LDS tile cells: 0 never, 1 automatic (>= 2048 particles per bin), 2 always
 *   tile_log2, tile_h_log2, bin_batch, unit_rows    tile / batch / unit geometry overrides (0 = automatic)
 *   k3_per_cu    persistent sort workgroups per CU          k1_general   1: always the general project+bin kernel
 *   k1_stack     fast project+bin kernel: -1 automatic, 0 / 1 project in place / through the wave stack
 *   ngp_general  1: no in-tile NGP fold                      dl_quot      0: no reciprocal-product grid quotient
 *   sort2        1: the two-level sort wherever a pass qualifies (default 0: the one-level sort)
 *   pending      chunks binned before one tile-kernel launch deposits them (0 = automatic: 8 ... 32)
 *   zero_batch   1 (default): the maps of a pass are cleared by one launch; 0: one hipMemsetAsync per map
 *   thin_host    1: shot-noise deviates (snopt > 0) drawn by libc rand() on the host, one call per selected entry;
 *                default 0: the process-global rand() stream continues on the device (slicer_libc_rand_supported)
 *   shear_split  1: every FFT of a slicer_shear handle created afterwards goes in passes of at most sqrt(length) points
 * Unknown keys return SLICER_ERR_ARG. */
int slicer_set_option(slicer_handle h, const char *key, int32_t value);
int slicer_get_option(slicer_handle h, const char *key, int32_t *value);

/* Shot-noise thinning (InputParams.snopt > 0) consumes the process-global libc rand() stream, one deviate per selected
 * entry (densitymaps.cpp:393).  The library continues that stream on the device: slicer_plane_begin of a pass with
 * snopt > 0 reads the generator state (before it touches the HIP runtime), the pass jumps and generates from that copy on
 * the GPU, and the advanced state is installed in libc when the pass ends -- before slicer_plane_flush / finalize / read
 * returns (or the next slicer_plane_begin, or slicer_destroy) -- so the caller's rand() calls after the pass see exactly
 * the stream position the reference would leave.  The host must not draw from rand() itself between plane_begin and
 * that point.  This needs glibc's default TYPE_3 generator (no initstate() with another size by the process) and passes
 * a layout self-check on a private state
 * array: 1 if so, 0 if thinning falls back to rand() calls on the host (same deviates, ~25x slower).  No GPU needed.
 * Reading and installing the state switches libc to a scratch state array for a few instructions (initstate / setstate):
 * like rand() itself next to srand(), not to be raced by rand() calls of other threads of the process.
 * CAUTION: once the HIP runtime runs, its own threads call rand() now and then (a kernel's first launch loads its code
 * object, allocations, ...), which moves the process-global stream at unpredictable points.  What they draw DURING a pass
 * is overwritten when the pass ends; what they draw between the host's own last draw and slicer_plane_begin (any HIP
 * work of the process in that window: creating the handle, other passes) is not.  A host that needs the reference's exact
 * thinning reads the stream BEFORE the first HIP call of the process (slicer_libc_rand_state_get needs no GPU) and gives
 * the handle its own copy (slicer_rand_stream_set below) -- what the createDensityMaps adapter and SLICER_amd do. */
int slicer_libc_rand_supported(void);
/* The process-global generator state as 31 words, oldest first (x[n-31] ... x[n-1] of x[n] = x[n-31] + x[n-3],
 * rand() = x[n] >> 1): read, and install.  Test hooks of the above; SLICER_ERR_UNSUPPORTED if not supported. */
int slicer_libc_rand_state_get(uint32_t *v31);
int slicer_libc_rand_state_set(const uint32_t *v31);
/* A stream of the handle's own for the shot-noise deviates, in the same 31-word form, instead of the process-global
 * one: the reference's MPI ranks each own an identically seeded copy of libc's stream and consume it independently
 * (densitymaps.cpp:187-217 seeds it in every rank alike); threads of ONE process that drive one device each get the same
 * by reading the process state once after the plan is made (slicer_libc_rand_state_get) and handing every handle a copy.
 * The handle's state advances with its draws (slicer_rand_stream_get reads it back); libc's own stream is not touched.
 * v31 = NULL returns the handle to the process-global stream.  Not inside a file. */
int slicer_rand_stream_set(slicer_handle h, const uint32_t *v31);
int slicer_rand_stream_get(slicer_handle h, uint32_t *v31);

/* The stream that this handle and every sub-handle made from it (slicer_kappa_*, slicer_smooth_*, ...) enqueue on.
 *   hip_stream   an existing hipStream_t of the handle's device, e.g. the caller framework's current stream.  NULL is
 *                the stream the handle created for itself (a blocking stream, what a new handle works on), NOT HIP's
 *                default stream: a handle never works on the default stream.  Its own stream is a blocking one, so it
 *                is ordered with the legacy default stream by HIP's rule for blocking streams.
 *   refused      null handle: SLICER_ERR_ARG.  Between slicer_plane_begin and slicer_plane_finalize (file open or
 *                not): SLICER_ERR_STATE -- a pass runs on one stream.  Accepted on a new handle and from
 *                slicer_plane_finalize on (slicer_plane_read finalizes, also where it ends in
 *                SLICER_ERR_NEGATIVE_COORD), while the maps of that pass stay readable.
 *   ordering     a call that changes the stream orders the new stream behind everything the handle and its sub-handles
 *                queued on the old one so far (one event recorded there, one hipStreamWaitEvent here; no host wait):
 *                maps finalized, tables uploaded by a *_create, results of a *_run on the old stream are complete
 *                for whatever is enqueued or read through the handle afterwards.  The old stream must still exist.
 *                A sub-handle has no stream of its own: "the stream of h" in the comments below is the one h has
 *                when the call is made, at its *_create and at every later call, so a sub-handle may be created
 *                before or after a switch.  Setting the stream it already has does nothing.  Work the CALLER queued on either stream is ordered
 *                by the streams themselves as usual. */
int slicer_set_stream(slicer_handle h, void *hip_stream);

/* ---- the deposit: hostile input -------------------------------------------------------------------------------------
 * What positions and masses that are not ordinary numbers do ("Non-finite and out-of-domain particles";
 * asserted by tests/test_gpu_hostile_particles.py against the oracle, value classes in tests/hostile_np.py).
 *   positions     Any f32 bit pattern is allowed.  Maps, per-type maps, nsel and the guard's return code are the
 *                 oracle's on every route.  The guard is any(x < 0 | y < 0 | z < 0) per particle, so a NaN never trips it;
 *                 a NaN coordinate fails the slab test or the field-of-view test and the particle drops out.  Deviation:
 *                 the reference's guard takes a min_element per axis, which a NaN as the FIRST element of an axis
 *                 silences; here a negative coordinate is reported wherever the NaN stands.
 *   masses, F32 / F64 (per-particle: hydro types with massarr == 0)
 *                 A mass that is NaN, negative or -inf has a NaN root: as in the reference its TSC footprint (3 x 3 pixels,
 *                 clipped to the map) becomes NaN.  The NaN pixels of every output map are exactly the oracle's, for NGP
 *                 also its +-inf pixels; on every other pixel the accumulator bounds hold against the exact sum over the
 *                 entries whose capped mass is finite and >= 0.  NaN payloads are not part of the contract.  (+inf,
 *                 like every mass above MAX_M = 1e3, counts as 0; 1000.0 exactly is kept.)
 *   masses, FIXED64
 *                 The integer accumulator cannot hold a NaN: a contribution that is not finite adds nothing, the words are
 *                 the sum of rint(c 2^e) over the finite contributions bit for bit, the map is finite everywhere, and nsel
 *                 still counts the entry.
 *   header masses massarr[t] of a type with npart[t] > 0 that is NaN, negative or infinite is refused by slicer_file_begin
 *                 with SLICER_ERR_ARG (the message names type and value): such a header is corrupt and would poison every
 *                 pixel the species touches.  0 stays what it is (hydro types: masses follow per particle).  A finite value
 *                 above MAX_M is deposited as is, as in the reference: the cap applies to per-particle masses only. */
int slicer_plane_begin(slicer_handle h, const slicer_plane_desc *desc);
int slicer_file_begin(slicer_handle h, const slicer_file_desc *file);
/* pos: AoS [n][3] f32 exactly as in the POS block (raw file units), host memory.  mass: per-particle
 * f32 masses (hydro types with massarr == 0: MASS / BHMA stream, densitymaps.cpp:358-372) or NULL. */
int slicer_deposit_host(slicer_handle h, int type, const float *pos, const float *mass, uint64_t n);
/* Same as slicer_deposit_host, but the library pulls the particles: `fill(user, dst_pos, dst_mass, first, count)`
 * must write particles [first, first+count) of this type straight into the pinned staging buffers it is given
 * (dst_mass is NULL when has_mass == 0) and return 0; e.g. an fread from the POS block.  Saves the pageable
 * copy of the whole block and overlaps file reads with H2D and kernels (double-buffered).  SURVEY S8f row N1. */
typedef int (*slicer_fill_fn)(void *user, float *dst_pos, float *dst_mass, uint64_t first, uint64_t count);
int slicer_deposit_stream(slicer_handle h, int type, uint64_t n, int has_mass, slicer_fill_fn fill, void *user);
/* same, operands already resident in this device's HBM */
int slicer_deposit_device(slicer_handle h, int type, const float *d_pos, const float *d_mass, uint64_t n);
int slicer_file_end(slicer_handle h);
int slicer_plane_finalize(slicer_handle h);

/* Device pointers of the finalized f32 maps of plane `plane` (npix*npix each): *d_tot, and
 * d_toti[0..5] (NULL for types that never appeared or when want_type_maps == 0). */
int slicer_plane_device_maps(slicer_handle h, int plane, float **d_tot, float **d_toti);
/* Synchronise, run the guard check, copy maps to host.  tot: npix^2 floats; toti: 6*npix^2 floats or
 * NULL; nsel: 6 int64 (true number of selected particles per type; the reference's own out-parameter
 * is always 0 because of the shadowed array at densitymaps.cpp:497) or NULL. */
int slicer_plane_read(slicer_handle h, int plane, float *tot, float *toti, int64_t *nsel);
int slicer_synchronize(slicer_handle h);
/* the hipStream_t all work of this handle is enqueued on, and the device array of selected-entry counters
 * of `plane` (6 x uint64), for callers that reduce across ranks themselves (slicer_amd_rccl.h) */
int slicer_get_stream(slicer_handle h, void **hip_stream);
int slicer_plane_info(slicer_handle h, int32_t *npix, int32_t *n_planes); /* of the current plane pass */
int slicer_plane_device_counts(slicer_handle h, int plane, uint64_t **d_counts);

/* Which deposit algorithms ran since slicer_plane_begin: bit SLICER_ALGO_DIRECT, bit SLICER_ALGO_BINNED
 * (1 << value), bit 3 = the shot-noise thinning kernels (snopt > 0); bits 4 / 5 tell which project+bin kernel the
 * binned path used (4: the f32-transform fast variant, 5: the general one; see slicer_project_bin.hip); bit 6: a tile
 * kernel launch kept its tiles as integer (u64) cells (constant-mass TSC, F32 / F64 accumulators, enough records per
 * tile; option k4_int = 0 / 2 forbids / forces them -- a tuning and test knob); bit 7: a chunk went through the two-level
 * sort (project+bin kernel sorts by coarse bin in LDS, k_sort2 by tile; option sort2 = 1 allows it); bit 8: shot-noise
 * deviates came from the device continuation of the libc stream. */
int slicer_plane_algo_mask(slicer_handle h, int32_t *mask);
/* Synchronise and report the negativity guard (densitymaps.cpp:334-345) without copying maps: SLICER_OK or
 * SLICER_ERR_NEGATIVE_COORD.  Callers that hand the device maps on (cross-rank reduce) call this first. */
int slicer_plane_status(slicer_handle h);

/* ---- cross-rank sum in the accumulator type ("reduce in the accumulator type, convert after") ----
 * Sequence per plane pass, on every rank, after the last slicer_file_end():
 *   slicer_plane_flush()              all deposits issued into the accumulators (no conversion yet)
 *   slicer_reduce_meta_get(&m)        which accumulators this rank holds + FIXED64 scales
 *   <combine m across ranks: element-wise MAX of m.v[], e.g. one small all-reduce>
 *   slicer_reduce_meta_set(&m)        allocates and zero-fills the accumulators this rank lacks, so that the SET OF
 *                                     COLLECTIVES IS THE SAME ON EVERY RANK (the reference reduces all 7 maps
 *                                     unconditionally, slicer-v2.cpp:214-217); fails if two ranks scaled the same
 *                                     FIXED64 accumulator differently
 *   slicer_plane_accumulators(p,...)  device pointers + element kind; sum them over ranks (ncclFloat / ncclDouble /
 *                                     ncclUint64: a FIXED64 N-rank sum is bitwise the 1-rank sum)
 *   slicer_plane_finalize()           on the root: accumulators -> f32 maps (once, after the sum)
 * slicer_amd_rccl.h wraps this sequence for RCCL; slicer_amd/parallel.py for torch.distributed. */
#define SLICER_REDUCE_META_INTS 24
typedef struct {
    /* v[0..6]   1 if accumulator slot s is live (s = type 0..5; s = 6: the shared all-types accumulator), else 0
     * v[7..13]  FIXED64 exponent of slot s, or INT32_MIN when not live / not FIXED64
     * v[14..20] minus that exponent, or INT32_MIN (so that an element-wise MAX exposes disagreeing ranks)
     * v[21]     negativity-guard flag of this rank (0/1)    v[22..23] reserved (0) */
    int32_t v[SLICER_REDUCE_META_INTS];
} slicer_reduce_meta;
int slicer_plane_flush(slicer_handle h);
int slicer_reduce_meta_get(slicer_handle h, slicer_reduce_meta *m);
int slicer_reduce_meta_set(slicer_handle h, const slicer_reduce_meta *m);
/* The same sequence without a host synchronisation (slicer_reduce_meta_get waits for the deposits in order to read the
 * negativity guard, which stalls a pipelined caller once per plane pass): _get_async fills in only what the host knows
 * (live accumulators, scales; v[21] = 0) and the caller combines the guard on the device instead -- one MAX all-reduce
 * of the int32 at *d_flag (slicer_plane_device_guard), issued with the map sums; slicer_plane_status /
 * slicer_plane_read then report a guard raised on any rank. */
int slicer_reduce_meta_get_async(slicer_handle h, slicer_reduce_meta *m);
int slicer_plane_device_guard(slicer_handle h, int32_t **d_flag);
/* acc[s] (s as above; NULL when not live), element kind SLICER_ELEM_* (one kind per pass), npix^2 elements each. */
int slicer_plane_accumulators(slicer_handle h, int plane, void **acc /* [7] */, int32_t *elem_kind);

/* --- utilities for benches and tests (device-side synthetic boxes) --- */
int slicer_device_malloc(slicer_handle h, size_t bytes, void **d_ptr);
int slicer_device_free(slicer_handle h, void *d_ptr);
int slicer_copy_to_device(slicer_handle h, void *d_dst, const void *src, size_t bytes);
int slicer_copy_to_host(slicer_handle h, void *dst, const void *d_src, size_t bytes);
int slicer_synth_positions(slicer_handle h, float *d_pos, uint64_t first, uint64_t count, double boxsize,
                           uint64_t seed, int clustered);
/* project only: writes xs, ys (and the plane index) of every selected entry of one chunk, in no
 * particular order, plus the source particle index; returns the count.  For parity tests of A1-A3. */
int slicer_debug_project(slicer_handle h, int type, const float *d_pos, uint64_t n, float *d_xs, float *d_ys,
                         int32_t *d_plane, uint64_t *d_src, uint64_t capacity, uint64_t *n_out);

/* debug: the device arithmetic primitives of the projection on arbitrary operands (device pointers, n doubles each).
 * op 0: out = sqrt(a)  (unscaled Newton iteration, valid for 2^-500 <= a <= 2^500)
 * op 1: out = a / b    (same operand range; a may be 0)
 * op 2: out = asin(a)  small-angle series, |a| <= 0.3125      op 3: out = atan(a), |a| <= 0.3125
 * op 4 / 5: the 9-term variants of 2 / 3, |a| <= 0.155
 * op 6 / 7: the raw hardware estimates v_rsq_f64(a), v_rcp_f64(a)      op 8 / 9: their one-step refinements
 *           (rsqrt_fast / rcp_fast of the fast project+bin kernel: not correctly rounded, < 2^-48 relative)
 * op 10: out = cell index floor((double)(float)a / dl) on a map of npix = (int)b & 0xFFFFF pixels (dl = 1 / npix, any
 *           npix: utilities.cpp:69-70)      op 11: TSC weight number ((int)b >> 20) & 3 (0, 1, 2) of that coordinate;
 *           bit 22 of b selects the reciprocal-product quotient a clean slicer_debug_dl_quotient sweep licenses
 *           (utilities.cpp:4-16, 82-88) -- the device evaluates both without the reference's f64 divisions except on
 *           exact ties
 * Lets the tests compare these with correctly rounded host results bit by bit (densitymaps.cpp:382-384 uses
 * sqrt, /, asin, atan2 of libm). */
int slicer_debug_math(slicer_handle h, int op, const double *d_a, const double *d_b, double *d_out, uint64_t n);

/* debug: the exhaustive sweep that licenses the f32 form of r / box in the fast project+bin kernel.  For every one of
 * the 2^31 non-negative binary32 values r whose fast quotient lies in the fast path's domain (0, or 2^-100..1) the
 * device compares it with (float)((double)r / box); *n_bad = number of mismatches (0 = licensed), examples8 = bit
 * patterns of up to eight offending r.  The library runs the same sweep once per handle and box size. */
int slicer_debug_box_quotient(slicer_handle h, double box, uint32_t *n_bad, uint32_t *examples8);
/* The same kind of proof for maps that are not a power of two wide: the grid arithmetic divides by dl = 1/npix in
 * f64 (utilities.cpp:69-70, :4-16); the device replaces the division by a reciprocal product + one FMA correction
 * (quot_dl3, slicer_device.hpp) for a map size only after this sweep -- every non-negative f32 operand below 2 against
 * the IEEE division, ~1 ms, run once per npix and handle -- found no mismatch.  n_bad = mismatches (0 expected). */
int slicer_debug_dl_quotient(slicer_handle h, int32_t npix, uint32_t *n_bad, uint32_t *examples8);

/* ---- Born-approximation convergence (kappa) maps ----
 * Weights, host only (no GPU): plane p has comoving edges ld[p] < ld2[p] (Mpc/h) and snapshot redshift zsnap[p]; the
 * background is flat w0waCDM with H0 = 100.  coeff[s * n_planes + p] = c_sp, the factor of (m_p - mean m_p) in
 * kappa_s = sum_p c_sp (m_p - mean m_p), m_p in 1e10 Msun/h per pixel; 0 for planes with z(ld2[p]) > zs[s] + 1e-4.
 * zs = NULL: the source redshifts are z(ld2[p]) of every plane (n_sources must equal n_planes).  growth = 0: no growth
 * correction D+(zl_p) / D+(zsnap[p]).  zlo, zup, zl, chil (n_planes each, any of them NULL): the edge redshifts, the
 * effective lens redshift and its comoving distance.  A curved background (|1 - omega_m - omega_lambda| > 1e-5) and
 * physical = 1 (a map size per plane) return SLICER_ERR_UNSUPPORTED; messages through slicer_last_error(NULL). */
int slicer_lensing_weights(double omega_m, double omega_lambda, double w0, double wa, double fov_deg, int32_t npix,
                           int32_t growth, int32_t physical, int32_t n_planes, const double *ld, const double *ld2,
                           const double *zsnap, int32_t n_sources, const double *zs, double *coeff, double *zlo,
                           double *zup, double *zl, double *chil);

/* Device accumulator of n_sources kappa maps of npix^2 pixels, on the device and stream of h (h's current one:
 * slicer_set_stream; destroy it before h).  Every call is enqueued on that stream with no host synchronisation, except
 * _plane_means and _read, which wait for it.
 *   slicer_kappa_add       n_maps (1..SLICER_MAX_PLANES) device f32 maps, e.g. slicer_plane_device_maps of a finalized
 *                          pass; coeff[m * n_sources + s] = c_sm (host memory, read before the call returns).  One read
 *                          of every map: A_s += sum_m c_sm m_m in f64, and the maps' f64 pixel sums -> their means.
 *   slicer_kappa_plane_means   the means of the first min(max, maps added) maps, in the order they were added
 *   slicer_kappa_finalize  kappa_s = A_s - sum_m c_sm mean_m, rounded once to f32; more maps may be added afterwards
 *                          (finalize again)
 *   slicer_kappa_device_map / _read    kappa_s of the last finalize (SLICER_ERR_STATE if maps were added after it)
 * The same call sequence gives bitwise the same maps.  The accumulators take n_sources * npix^2 * 12 bytes
 * (SLICER_ERR_NOMEM). */
typedef struct slicer_kappa_s *slicer_kappa_handle;
int slicer_kappa_create(slicer_handle h, int32_t npix, int32_t n_sources, slicer_kappa_handle *out);
int slicer_kappa_add(slicer_kappa_handle kh, int32_t n_maps, const float *const *d_maps, const double *coeff);
int slicer_kappa_plane_means(slicer_kappa_handle kh, double *out, int32_t max);
int slicer_kappa_finalize(slicer_kappa_handle kh);
int slicer_kappa_device_map(slicer_kappa_handle kh, int32_t s, float **d_map);
int slicer_kappa_read(slicer_kappa_handle kh, int32_t s, float *host);
int slicer_kappa_destroy(slicer_kappa_handle kh);

/* ---- Lensing potential and shear maps from a kappa map ----
 * For an npix^2 map kappa (row i0 slow, i1 contiguous) of side theta = angle_deg * pi / 180 radians, d = theta / npix:
 * K0 = 2 pi fftfreq(npix, d) along i0, K1 = 2 pi rfftfreq(npix, d) along i1, k^2 = K0^2 + K1^2 (every quotient 0 at 0),
 *   khat = rfft2(kappa);  phi = irfft2(-2 khat / k^2);  gamma1 = irfft2(khat (K0^2 - K1^2) / k^2);
 *   gamma2 = irfft2(khat 2 K0 K1 / k^2);  |gamma| = sqrt(gamma1^2 + gamma2^2),  irfft2 with s = (npix, npix),
 * computed in f64 and rounded once to f32, on the device and stream of h (h's current one: slicer_set_stream;
 * destroy it before h).  Supported: 2 <= npix <= 16384 with prime factors 2, 3, 5, 7 only (slicer_shear_supported, host
 * only); others return SLICER_ERR_UNSUPPORTED.  angle_deg <= 0 or not finite: SLICER_ERR_ARG.
 *   slicer_shear_run         any device f32 npix^2 map (e.g. slicer_kappa_device_map); enqueued, no synchronisation
 *   slicer_shear_spectrum    khat of the last run, [npix][npix/2+1] (re, im) f64 pairs; waits for the stream
 *   slicer_shear_device_map / _read   map `which` (SLICER_SHEAR_*) of the last run (SLICER_ERR_STATE before any run);
 *                            _read waits for the stream
 * Option shear_split = 1 (slicer_set_option, read at create) splits every transform into passes of at most
 * sqrt(length) points, the path that longer maps take.  The same input gives bitwise the same maps.  Device memory:
 * about 4 f64 complex npix x (npix/2+1) arrays plus the four f32 maps (SLICER_ERR_NOMEM). */
#define SLICER_SHEAR_PHI 0
#define SLICER_SHEAR_GAMMA1 1
#define SLICER_SHEAR_GAMMA2 2
#define SLICER_SHEAR_GAMMA 3
int slicer_shear_supported(int32_t n);
typedef struct slicer_shear_s *slicer_shear_handle;
int slicer_shear_create(slicer_handle h, int32_t npix, double angle_deg, slicer_shear_handle *out);
int slicer_shear_run(slicer_shear_handle sh, const float *d_kappa);
int slicer_shear_spectrum(slicer_shear_handle sh, double *host);
int slicer_shear_device_map(slicer_shear_handle sh, int32_t which, float **d_map);
int slicer_shear_read(slicer_shear_handle sh, int32_t which, float *host);
int slicer_shear_destroy(slicer_shear_handle sh);

/* ---- Deflection maps, and the finite-difference derivatives of a potential map ----
 * Spectral deflection alpha = grad phi, in the notation of N6 (phihat = -2 khat / k^2, 0 at k = 0):
 *   alpha1 = irfft2(i K0 phihat);  alpha2 = irfft2(i K1 phihat),  s = (npix, npix), in radians,
 * computed in f64 and rounded once to f32; irfft2's Hermitian projection of the columns k1 = 0 and k1 = npix/2 decides
 * what becomes of row and column npix/2, as for the maps of N6.
 *   slicer_shear_deflection  both maps from the spectrum of the last slicer_shear_run (two inverse transforms, no forward
 *                            one); enqueued, no synchronisation.  Before any run: SLICER_ERR_STATE.  The two f32 maps
 *                            are allocated by the first call (SLICER_ERR_NOMEM); the maps of N6 and the spectrum are
 *                            left as they are.
 *   slicer_shear_device_map / _read with SLICER_SHEAR_ALPHA1 / _ALPHA2: SLICER_ERR_STATE until slicer_shear_deflection
 *                            has followed the last slicer_shear_run.  shear_split = 1 gives bitwise the same maps.
 * Finite differences (the real-space mode of the reference's smr.smr(..., derivative="gradient"); a light-cone map is not
 * periodic, and these stencils do not wrap its edges).  On a line f of n >= 5 samples of spacing d:
 *   D1 f[i] = (f[i-2] - 8 f[i-1] + 8 f[i+1] - f[i+2]) / (12 d)                 for 2 <= i <= n-3,
 *             (f[i+1] - f[i]) / d  at i = 0, 1  and  (f[i] - f[i-1]) / d  at i = n-2, n-1;
 *   D2 f[i] = (-f[i-2] + 16 f[i-1] - 30 f[i] + 16 f[i+1] - f[i+2]) / (12 d^2)   for 2 <= i <= n-3,
 *             (2 f[i] - 5 f[i+1] + 4 f[i+2] - f[i+3]) / d^2  at i = 0, 1  and its mirror image at i = n-2, n-1.
 * From an f32 npix^2 map phi (axis 0 slow, axis 1 contiguous): ALPHA1 = D1 along axis 0, ALPHA2 = D1 along axis 1,
 * p11 = D2 along axis 0, p22 = D2 along axis 1, p12 = D1 along axis 1 of D1 along axis 0 (equal to the other order),
 * KAPPA = (p11 + p22) / 2, GAMMA1 = (p11 - p22) / 2, GAMMA2 = p12, GAMMA = sqrt(GAMMA1^2 + GAMMA2^2); everything in f64
 * from the f32 samples, each output rounded once to f32.  Any npix from 5 to 524288: no restriction on its factors.
 *   slicer_fd_derivatives    one kernel on the stream of h; enqueued, no synchronisation.  d_out[SLICER_FD_*]: device
 *                            buffers of npix^2 floats owned by the caller; NULL entries are skipped.  SLICER_ERR_ARG:
 *                            npix outside 5..524288, a spacing that is not positive and finite, a NULL input, every
 *                            output NULL, an output equal to the input.  The same input gives bitwise the same maps,
 *                            wherever the pointers lie and whichever outputs are asked for.
 *   slicer_shear_fd          the same of the handle's f32 phi of the last slicer_shear_run with d = theta / npix, into six
 *                            maps of the handle's, allocated by the first call (SLICER_ERR_NOMEM); read with
 *                            SLICER_SHEAR_FD_ALPHA1 ... _FD_GAMMA under the state rule of the deflection maps.  Before
 *                            any run: SLICER_ERR_STATE; a handle of npix < 5: SLICER_ERR_UNSUPPORTED.
 * The `which` codes 4 ... 7 and 10 ... 15 name nothing (SLICER_ERR_ARG). */
#define SLICER_SHEAR_ALPHA1 8
#define SLICER_SHEAR_ALPHA2 9
#define SLICER_FD_ALPHA1 0
#define SLICER_FD_ALPHA2 1
#define SLICER_FD_KAPPA 2
#define SLICER_FD_GAMMA1 3
#define SLICER_FD_GAMMA2 4
#define SLICER_FD_GAMMA 5
#define SLICER_FD_COUNT 6
#define SLICER_SHEAR_FD_ALPHA1 16 /* SLICER_SHEAR_FD_ALPHA1 + SLICER_FD_*: */
#define SLICER_SHEAR_FD_ALPHA2 17
#define SLICER_SHEAR_FD_KAPPA 18
#define SLICER_SHEAR_FD_GAMMA1 19
#define SLICER_SHEAR_FD_GAMMA2 20
#define SLICER_SHEAR_FD_GAMMA 21
int slicer_shear_deflection(slicer_shear_handle sh);
int slicer_shear_fd(slicer_shear_handle sh);
int slicer_fd_derivatives(slicer_handle h, int32_t npix, double spacing, const float *d_phi,
                          float *const d_out[SLICER_FD_COUNT]);

/* ---- Binned auto and cross power spectra of kappa maps ----
 * For n_maps maps kappa_s of npix^2 pixels (row i0 slow, i1 contiguous) of side theta = angle_deg * pi / 180 radians:
 * khat_s = rfft2(kappa_s) in f64 on the [npix][npix/2+1] half plane (the spectrum of slicer_shear_run).  Mode (i0, i1)
 * has j0 = the signed fftfreq index of i0, j1 = i1, the integer m2 = j0^2 + j1^2 and ell = l_f sqrt(m2), with
 * l_f = 2 pi / theta.  Edges r_0 < ... < r_B are radii in units of l_f; a mode is in bin b iff
 * r_b * r_b <= m2 < r_{b+1} * r_{b+1} (the squares rounded to f64), the last bin closed on the right; other modes are
 * dropped.  edges = NULL: 0, 1, ..., npix-1 (n_edges must then be npix).  Every half-plane coefficient is one mode.
 *   counts[b] = N_b,  mean_radius[b] = mean of sqrt(m2) over the bin (NaN if N_b = 0),
 *   C_st,b = theta^2 / npix^4 * (1 / N_b) * sum over the bin of Re(khat_s conj khat_t)   (NaN if N_b = 0).
 *   slicer_power_bins      N_b and the mean radii, host only (no device); messages through slicer_last_error(NULL)
 *   slicer_power_create    on the device and stream of h (h's current one: slicer_set_stream, destroy it before h);
 *                          reads the shear_split option.  cross = 0: the n_maps auto-spectra; cross = 1: all
 *                          n_maps (n_maps + 1) / 2 pairs (0,0), (0,1), ..., (0,S-1), (1,1), ...  Refused before any
 *                          allocation: npix that slicer_shear_supported rejects or n_maps outside 1..128
 *                          (SLICER_ERR_UNSUPPORTED); bad edges (fewer than 2, negative, not finite, not strictly
 *                          ascending) or an angle that is not positive and finite (SLICER_ERR_ARG).  Device memory:
 *                          the transform's buffers plus one (cross = 0) or n_maps (cross = 1) spectra of
 *                          16 npix (npix/2+1) bytes (SLICER_ERR_NOMEM).
 *   slicer_power_run       n_maps device f32 maps (e.g. slicer_kappa_device_map); enqueued, no synchronisation
 *   slicer_power_spectrum  khat of map `map` of the last run, [npix][npix/2+1] (re, im) f64 pairs, bitwise equal to
 *                          slicer_shear_spectrum under the same shear_split; with cross = 0 only the last map's is kept
 *                          (others: SLICER_ERR_STATE); waits for the stream
 *   slicer_power_read      cl [pairs][n_edges-1], ell_mean = l_f * mean_radius and counts [n_edges-1] of the last run
 *                          (any of them NULL); waits for the stream.  Before any run: SLICER_ERR_STATE.
 * No atomics: the same maps give bitwise the same spectra, and C_ss is the same with cross = 0 and cross = 1. */
int slicer_power_bins(int32_t npix, int32_t n_edges, const double *edges, int64_t *counts, double *mean_radius);
typedef struct slicer_power_s *slicer_power_handle;
int slicer_power_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_maps, int32_t cross,
                        int32_t n_edges, const double *edges, slicer_power_handle *out);
int slicer_power_run(slicer_power_handle ph, const float *const *d_maps);
int slicer_power_spectrum(slicer_power_handle ph, int32_t map, double *host);
int slicer_power_read(slicer_power_handle ph, double *cl, double *ell_mean, int64_t *counts);
int slicer_power_destroy(slicer_power_handle ph);

/* ---- Central moments of a map over a pyramid of 2x2 halvings ----
 * Level 0 is the caller's f32 map of npix^2 pixels (row-major); level l+1 has n_{l+1} = n_l / 2 (integer division: for odd
 * n_l the last row and column do not enter it) and, in f32 and in this order (Lens/halve.py),
 *   y[i][j] = ((x[2i][2j] + x[2i+1][2j]) + x[2i][2j+1]) + x[2i+1][2j+1],
 * stored as it is (SLICER_HALVE_SUM, for mass planes) or as 0.25f * y (SLICER_HALVE_MEAN, for kappa); no FMA.
 * Of every level, over ALL its N = n_l^2 pixels (the row and column that halving drops included), about a centre c (f64):
 *   d_i = (double)x_i - c,  p_2 = d * d,  p_k = p_{k-1} * d,  S_k = sum_i p_k(i)  for k = 2 ... 8  (Lens/moment.py),
 * each operation rounded once to f64, summed in f64 in a fixed tree, and the mean mu = (sum_i x_i) / N likewise.  No
 * atomics: the same input gives bitwise the same numbers.  The raw sums are returned, not S_k / N: the moment of F
 * realisations is m_k = sum_f S_k(f) / (F N), as moment.py averages them.
 * Centre of level l: centres[l], or the level's own device mean where centres[l] is NaN or centres is NULL.
 * Pyramid against one level: of slicer_moments_read's fields, `sums`, `centres_used` and `npix_level` of level l are
 * always bitwise those of a levels = 0 run on the level-l map with the same centre.  `means` of level l is bitwise that
 * run's too when the levels = 0 run is given no centre (NULL or NaN): the mean of a map comes from a sum pass of its
 * own, in the order in which a halving pass writes that map.  When the levels = 0 run is GIVEN its centre, the map is
 * read once, no such pass runs, and its mean is summed along with the S_k, in their tree: `means` then agrees with the
 * pyramid's within the mean's bound below, not bitwise.  The same holds for level 0 of any run with centres[0] given.
 * Tree depth: D(n) = slicer_moments_depth(n) is the number of f64 additions on the longest path of either tree of an
 * n x n level.  With ceil-divisions, T = (n/2) ceil((n/2)/2) + (n odd ? ceil((2n-1)/8) : 0), U = n ceil(n/2):
 *   D(n) = max( 8 min(8, ceil(T / 256)) + 18 + ceil(ceil(T / 2048) / 256),
 *               2 min(8, ceil(U / 256)) + 18 + ceil(ceil(U / 2048) / 256) );         D(16384) = 290.
 * Bounds, u = 2^-53, A_k = sum_i |x_i - c|^k:  |S_k - exact| <= (2k - 1 + D) u (1 + 2^-20) A_k  (the rounding of d
 * k-fold, k - 1 products, D additions);  |mu - exact| <= (D + 2) u mean|x_i|.
 *   slicer_moments_depth     D(npix), host only; -1 for npix outside 1..131072 (message through slicer_last_error(NULL))
 *   slicer_moments_create    on the device and stream of h (h's current one: slicer_set_stream, destroy it before
 *                            h); allocates the level maps.  The numbers are checked before the handle, so that they
 *                            can be checked without a device: npix < 1, levels outside 0..floor(log2 npix), a mode that
 *                            is neither SLICER_HALVE_*: SLICER_ERR_ARG; npix > 131072: SLICER_ERR_UNSUPPORTED
 *   slicer_moments_run       any device f32 npix^2 map (e.g. slicer_kappa_device_map), which is only read; centres:
 *                            NULL or levels + 1 doubles in host memory, read before the call returns; enqueued, no
 *                            synchronisation, no host round trip between the levels
 *   slicer_moments_read      n_l [levels+1], mu_l [levels+1], the centres used [levels+1], S_k [levels+1][7] of the last
 *                            run (any of them NULL); waits for the stream.  Before any run: SLICER_ERR_STATE
 *   slicer_moments_device_map / _read_map   level 1 ... levels of the last run (other levels: SLICER_ERR_ARG; before
 *                            any run: SLICER_ERR_STATE); _read_map waits for the stream */
typedef struct slicer_moments *slicer_moments_handle;
#define SLICER_MOMENTS_ORDERS 7 /* k = 2 ... 8 */
enum { SLICER_HALVE_MEAN = 0, SLICER_HALVE_SUM = 1 };
int slicer_moments_depth(int32_t npix);
int slicer_moments_create(slicer_handle h, int32_t npix, int32_t levels, int32_t mode, slicer_moments_handle *out);
int slicer_moments_run(slicer_moments_handle mh, const float *d_map, const double *centres);
int slicer_moments_read(slicer_moments_handle mh, int32_t *npix_level, double *means, double *centres_used,
                        double *sums);
int slicer_moments_device_map(slicer_moments_handle mh, int32_t level, float **d_map);
int slicer_moments_read_map(slicer_moments_handle mh, int32_t level, float *host);
int slicer_moments_destroy(slicer_moments_handle mh);

/* ---- One-point PDF histogram and peak / minimum counts of a map ----
 * The input is any device f32 map of npix^2 pixels (row-major), 1 <= npix <= 131072, which is only read.  The edges
 * e_0 < e_1 < ... < e_B are f64, finite and strictly ascending, 1 <= B <= SLICER_PEAKS_MAX_BINS.
 * PDF: every pixel x is widened exactly to f64 and compared in f64 against the f64 edges (the edges are never rounded
 * to f32).  x is in bin b iff e_b <= x < e_{b+1}; the last bin is closed, x = e_B is in bin B-1 (numpy.histogram's
 * rule).  x < e_0 or -inf counts as `below`, x > e_B or +inf as `above`, NaN as `nan`; the four kinds sum to npix^2.
 * Peaks and minima: a candidate is a pixel (i, j) with 1 <= i, j <= npix-2 (the map is a field of view and does not
 * wrap: border pixels are never candidates, and for npix < 3 there are none).  It is a peak iff it is strictly greater
 * than each of its 8 neighbours, a minimum iff strictly less than each, compared in f32.  Ties give neither (a plateau
 * has no peaks); every comparison with a NaN is false, so a NaN pixel and each of its neighbours is neither.  Peaks and
 * minima are each histogrammed by the pixel's own value over the same edges by the same rule, with `below` and `above`
 * counts of their own.
 * All counts are int64 and exact; the same input gives the same numbers on every run; there is no floating-point
 * accumulation anywhere.  `below` and `above` are indexed 0 = pdf, 1 = peaks, 2 = minima.
 *   slicer_peaks_edges      host only: e_0 = lo, e_B = hi, e_b = lo + b * ((hi - lo) / B) for 0 < b < B, each operation
 *                           rounded once to f64, no FMA.  SLICER_ERR_ARG (message through slicer_last_error(NULL)):
 *                           bins outside 1..1024, lo or hi not finite, a NULL array, edges that are not finite and
 *                           strictly ascending after rounding
 *   slicer_peaks_create     on the device and stream of h (h's current one: slicer_set_stream, destroy it before h).
 *                           The numbers are checked before the handle, so that they can be checked without a device:
 *                           npix < 1, fewer than 2 or more than 1025 edges, an edge that is not finite, edges not
 *                           strictly ascending: SLICER_ERR_ARG; npix > 131072: SLICER_ERR_UNSUPPORTED.  Device memory:
 *                           the edges, 8 (3 B + 7) bytes of results and at most max(64, 8 per compute unit) rows of
 *                           4 (3 B + 7) bytes (SLICER_ERR_NOMEM)
 *   slicer_peaks_run        any device f32 map of the handle's npix^2 pixels (e.g. slicer_kappa_device_map); enqueued, no
 *                           synchronisation.  A NULL map: SLICER_ERR_ARG
 *   slicer_peaks_run_npix   the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                           SLICER_ERR_ARG), so that one handle serves every level of a moments pyramid
 *                           (slicer_moments_device_map)
 *   slicer_peaks_read       pdf, peaks, minima [B] each, below [3], above [3], the NaN count, of the last run (any of
 *                           them NULL); waits for the stream.  Before any run: SLICER_ERR_STATE */
typedef struct slicer_peaks *slicer_peaks_handle;
#define SLICER_PEAKS_MAX_BINS 1024
int slicer_peaks_edges(double lo, double hi, int32_t bins, double *edges);
int slicer_peaks_create(slicer_handle h, int32_t npix, int32_t n_edges, const double *edges, slicer_peaks_handle *out);
int slicer_peaks_run(slicer_peaks_handle ph, const float *d_map);
int slicer_peaks_run_npix(slicer_peaks_handle ph, const float *d_map, int32_t npix);
int slicer_peaks_read(slicer_peaks_handle ph, int64_t *pdf, int64_t *peaks, int64_t *minima, int64_t *below,
                      int64_t *above, int64_t *n_nan);
int slicer_peaks_destroy(slicer_peaks_handle ph);

/* ---- Minkowski functionals of a map's excursion sets, as exact counts ----
 * The input is any device f32 map of npix^2 pixels (row-major), 1 <= npix <= 131072, which is only read.  The thresholds
 * t_0 < t_1 < ... < t_{T-1} are f64, finite and strictly ascending, 1 <= T <= SLICER_MINKOWSKI_MAX_THRESHOLDS (the B + 1
 * edges of slicer_peaks_edges with B <= 1024 serve as thresholds).
 * Rank: k(x) = the number of t_j <= x, every pixel x widened exactly to f64 and compared in f64 against the f64 thresholds
 * (the thresholds are never rounded to f32); k(NaN) = 0, k(-inf) = 0, k(+inf) = T.  Pixel x is in the excursion set Q_j
 * (x >= t_j) iff k(x) > j.  A NaN is in no set; the NaN pixels are counted in n_nan.
 * Pixel complex: the map is npix^2 closed unit squares (faces), 2 npix (npix + 1) unit edges and (npix + 1)^2 vertices.
 * The field of view does not wrap; positions outside the map are in no set (rank 0).  An edge or a vertex belongs to the
 * closure of Q_j iff at least one of its adjacent faces does: an edge has 2 adjacent faces, an edge on the map's border 1,
 * a vertex 4, 2 or 1.  Per threshold j = 0 ... T-1:
 *   faces[j]     the pixels with k > j
 *   edges[j]     the edges, border edges included, with max k over their adjacent faces > j
 *   vertices[j]  the vertices with max k over their adjacent faces > j
 *   boundary[j]  the interior edges with exactly one of their two faces in Q_j (max k > j and not min k > j): the
 *                perimeter of Q_j inside the field, in pixel sides
 *   border[j]    the border edges whose one face is in Q_j: the part of the outline that lies on the map's rim (a corner
 *                pixel counts twice); kept apart from boundary so that the caller chooses the convention
 * The Euler characteristic chi[j] = vertices[j] - edges[j] + faces[j] is the number of 8-connected components of Q_j minus
 * its holes (the 4-connected components of the complement that do not reach outside the map); it is not stored here.
 * All counts are int64 and exact; the same input gives the same numbers on every run; there is no floating-point
 * accumulation anywhere.
 *   slicer_minkowski_create    on the device and stream of h (h's current one: slicer_set_stream, destroy it before
 *                              h).  The numbers are checked before the handle, so that they can be checked without a
 *                              device: npix < 1, fewer than 1 or more than 1025 thresholds, a threshold that is not
 *                              finite, thresholds not strictly ascending: SLICER_ERR_ARG; npix > 131072:
 *                              SLICER_ERR_UNSUPPORTED.  Device memory: the thresholds, 8 (5 T + 1) + 8 (5 (T + 1) + 1)
 *                              bytes of results and at most max(64, 8 per compute unit) rows of 4 (5 (T + 1) + 1) bytes
 *                              (SLICER_ERR_NOMEM)
 *   slicer_minkowski_run       any device f32 map of the handle's npix^2 pixels (e.g. slicer_kappa_device_map);
 *                              enqueued, no synchronisation.  A NULL map: SLICER_ERR_ARG
 *   slicer_minkowski_run_npix  the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                              SLICER_ERR_ARG), so that one handle serves every level of a moments pyramid
 *   slicer_minkowski_read      faces, edges, vertices, boundary, border [T] each and the NaN count of the last run (any
 *                              of them NULL); waits for the stream.  Before any run: SLICER_ERR_STATE */
typedef struct slicer_minkowski *slicer_minkowski_handle;
#define SLICER_MINKOWSKI_MAX_THRESHOLDS 1025
int slicer_minkowski_create(slicer_handle h, int32_t npix, int32_t n_thresholds, const double *thresholds,
                            slicer_minkowski_handle *out);
int slicer_minkowski_run(slicer_minkowski_handle mh, const float *d_map);
int slicer_minkowski_run_npix(slicer_minkowski_handle mh, const float *d_map, int32_t npix);
int slicer_minkowski_read(slicer_minkowski_handle mh, int64_t *faces, int64_t *edges, int64_t *vertices, int64_t *boundary,
                          int64_t *border, int64_t *n_nan);
int slicer_minkowski_destroy(slicer_minkowski_handle mh);

/* ---- Binned bispectra of a kappa map ----
 * In the notation of the power spectra above (row N7): theta = angle_deg * pi / 180, khat = rfft2(kappa) in f64,
 * l_f = 2 pi / theta, edges r_0 < ... < r_B in units of l_f (edges = NULL: 0, 1, ..., npix-1 with n_edges = npix), and a
 * mode is in bin b by the rule of slicer_power_bins: r_b * r_b <= m2 < r_{b+1} * r_{b+1} on the integer m2, the squares
 * rounded to f64, the last bin closed on the right.  One exception: the mode m2 = 0 is in no bin (the mean never enters a
 * bispectrum).  Per bin b, both kept in f64 and never rounded to f32 (the normalisation below cancels heavily for thin
 * triangles):
 *   F_b = irfft2(khat * 1[mode in b]),   I_b = irfft2(1[mode in b]),   s = (npix, npix)
 * and per triple i <= j <= k of bins
 *   S_ijk = sum over the pixels of F_i F_j F_k,   T_ijk = npix^4 * sum over the pixels of I_i I_j I_k,
 *   B_ijk = theta^4 / npix^6 * (npix^4 S_ijk) / T_ijk          (the convention of C = theta^2 / npix^4 |khat|^2).
 * In exact arithmetic T_ijk is an integer: the number of ordered triples (l1 in i, l2 in j, l3 in k) of modes of the full
 * npix x npix plane with l1 + l2 + l3 = 0 modulo npix on both axes, and npix^4 S_ijk is the sum of
 * khat(l1) khat(l2) khat(l3) over those same triangles.  Triangles that close only modulo npix are counted by S and by T
 * alike; edges at or below npix / 3 avoid them.  A triple whose T reads below 0.5 has no closed triangle: its B is NaN.
 * A triple list is n_triples rows (i, j, k) of int32 with 0 <= i <= j <= k < B (otherwise SLICER_ERR_ARG); it may repeat
 * a triple.  triples = NULL: all B (B + 1) (B + 2) / 6 triples in lexicographic order (n_triples must be that number).
 *   slicer_bispectrum_triangles  the exact T of every triple of the list, host only (no device; messages through
 *                                slicer_last_error(NULL)): an enumeration of the modes of bins i and j with a table
 *                                lookup of -l1 - l2.  Bad edges are refused as by slicer_power_bins, npix outside
 *                                1..16384 and a bad triple with SLICER_ERR_ARG; more than 2^31 mode pairs (the sum of
 *                                N_i N_j over the triples, N the full-plane modes of a bin): SLICER_ERR_UNSUPPORTED
 *   slicer_bispectrum_create     on the device and stream of h (h's current one: slicer_set_stream, destroy it before
 *                                h); reads the shear_split option.  Refused before any allocation: an npix that
 *                                slicer_shear_supported rejects, more than 32 bins or more than 2^20 triples
 *                                (SLICER_ERR_UNSUPPORTED); bad edges, a bad triple, an angle that is not positive and
 *                                finite (SLICER_ERR_ARG).  T is computed here, once, on the device, from the I_b in the
 *                                buffer that the runs then use for the F_b; it waits for the stream.  Device memory
 *                                (SLICER_ERR_NOMEM): B maps of 8 npix^2 bytes, one spectrum of 16 npix (npix/2+1) bytes,
 *                                the transform's buffers, and 8 n_triples bytes per chunk of pixels (at most 1024 chunks,
 *                                of at least 4096 pixels)
 *   slicer_bispectrum_run        a device f32 map (e.g. slicer_kappa_device_map); enqueued, no synchronisation
 *   slicer_bispectrum_read       b, triangles (the T as the device summed them, not rounded) and sums (the raw S),
 *                                [n_triples] each, any of them NULL; waits for the stream.  triangles can be read right
 *                                after create; b and sums before any run: SLICER_ERR_STATE
 *   slicer_bispectrum_spectrum   khat of the last run, [npix][npix/2+1] (re, im) f64 pairs, bitwise equal to
 *                                slicer_shear_spectrum under the same shear_split; waits for the stream
 *   slicer_bispectrum_read_map   F_bin of the last run, [npix][npix] f64; waits for the stream
 * No atomics: the same input gives bitwise the same output, run after run; the S of a triple does not depend on which
 * other triples are in the list; an input pointer off the 16-byte grid gives the same bits; shear_split 0 and 1 give the
 * same bits of b, triangles, sums and the maps.  (shear_split reorders the transform's butterflies and with them the last
 * bits of slicer_shear_spectrum, so every result here comes from the unsplit plan; with shear_split = 1 the map is
 * transformed once more with the split plan, and that is the spectrum slicer_bispectrum_spectrum reports: it differs
 * from the one behind the results by the transform's rounding, and costs a second plan's buffers.)  Products
 * associate as (F_i F_j) F_k; the sums are blocked (64 products, then the blocks of a chunk, a butterfly over 64 lanes,
 * then the chunks in index order in 64 runs and a second butterfly). */
typedef struct slicer_bispectrum_s *slicer_bispectrum_handle;
#define SLICER_BISPECTRUM_MAX_BINS 32
int slicer_bispectrum_triangles(int32_t npix, int32_t n_edges, const double *edges, int32_t n_triples,
                                const int32_t *triples /* [n_triples][3] or NULL */, int64_t *out);
int slicer_bispectrum_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_edges, const double *edges,
                             int32_t n_triples, const int32_t *triples, slicer_bispectrum_handle *out);
int slicer_bispectrum_run(slicer_bispectrum_handle bh, const float *d_map);
int slicer_bispectrum_read(slicer_bispectrum_handle bh, double *b, double *triangles, double *sums);
int slicer_bispectrum_spectrum(slicer_bispectrum_handle bh, double *host);
int slicer_bispectrum_read_map(slicer_bispectrum_handle bh, int32_t bin, double *host);
int slicer_bispectrum_destroy(slicer_bispectrum_handle bh);

/* ---- Multi-plane ray tracing through the lens planes ----
 * One ray per pixel of an npix^2 grid (axis 0 slow = component 1, axis 1 contiguous = component 2, as for N6 and N8), on the
 * device and stream of h (h's current one: slicer_set_stream, destroy it before h).  State per ray, 12 f64: position
 * b = (b1, b2) and direction t = (t1, t2) in pixel units, centred (b = beta / d, d = the spacing in radians per pixel,
 * h = (npix - 1) / 2), and the 2 x 2 matrices A = d beta / d theta and T = d t / d theta.  Start: the ray of pixel (i, j)
 * has b = t = (i - h, j - h), A = T = I; the last plane distance is chi = 0.  Every operation below is one IEEE f64
 * operation rounded once (RN), in this order, with no FMA: a host restatement reproduces the device bit for bit.
 * Step to the plane at comoving distance chi_k > chi_{k-1}, described by five f32 maps of npix^2 (alpha1, alpha2 in radians,
 * kappa, gamma1, gamma2: the maps of N6 / N8 of that plane's lens map), with w = RN(RN(chi_k - chi_{k-1}) / chi_k):
 *   1. b_a <- RN(b_a + RN(w RN(t_a - b_a)));  A_ab <- RN(A_ab + RN(w RN(T_ab - A_ab)))
 *   2. u_a = RN(b_a + h), i_a = floor(u_a), f_a = RN(u_a - i_a), g_a = RN(1 - f_a).  The cell's corners are i_a mod npix and
 *      (i_a + 1) mod npix, the mathematical modulo: the grid wraps.  A ray with a u that is not finite or has |u| >= 2^30 in
 *      either component reads pixel (0, 0) with f1 = f2 = NaN: its state becomes NaN and stays NaN; no other ray is affected.
 *   3. per map, with the four samples m00 at (i1, i2), m01 at (i1, i2+1), m10 at (i1+1, i2), m11 at (i1+1, i2+1) widened to
 *      f64:  r0 = RN(RN(g2 m00) + RN(f2 m01)),  r1 = RN(RN(g2 m10) + RN(f2 m11)),  v = RN(RN(g1 r0) + RN(f1 r1))
 *   4. U11 = RN(v_kappa + v_gamma1), U22 = RN(v_kappa - v_gamma1), U12 = U21 = v_gamma2
 *   5. t_a <- RN(t_a - RN(v_alpha_a / d))
 *   6. T_ab <- RN(T_ab - RN(RN(U_a1 A_1b) + RN(U_a2 A_2b)))   with the A of step 1
 * Observe at chi_s >= chi of the last plane, w_s = RN(RN(chi_s - chi) / chi_s): bs and As are step 1 with w_s (the state is
 * not changed); six f32 maps, each formed in f64 and rounded once to f32:
 *   kappa = 1 - RN(0.5 RN(As11 + As22)),  gamma1 = 0.5 RN(As22 - As11),  gamma2 = -0.5 RN(As12 + As21),
 *   omega = 0.5 RN(As21 - As12),  deflection_a = RN(RN(theta_a - bs_a) d) in radians,  theta = (i - h, j - h),
 * the convention A = [[1 - kappa - gamma1, -gamma2 - omega], [-gamma2 + omega, 1 - kappa + gamma1]].  The sign and
 * payload of a NaN result are not part of the contract.
 *   slicer_rays_create    allocates the twelve state arrays, 96 bytes per ray (SLICER_ERR_NOMEM); launches nothing.  The
 *                         numbers are checked before the handle, so that they can be checked without a device: npix < 1, a
 *                         spacing that is not positive and finite: SLICER_ERR_ARG; npix > 131072: SLICER_ERR_UNSUPPORTED
 *   slicer_rays_reset     back to the start state; nothing launched
 *   slicer_rays_step      one kernel; enqueued, no synchronisation; the maps are only read.  SLICER_ERR_ARG: chi not finite
 *                         or not above the last plane's, a NULL map
 *   slicer_rays_observe   one kernel; enqueued, no synchronisation.  d_out[SLICER_RAYS_*]: device buffers of npix^2 floats
 *                         owned by the caller, NULL entries are skipped.  Allowed before any step (zeros).  SLICER_ERR_ARG:
 *                         chi_s not positive and finite or below the last plane's, every output NULL
 *   slicer_rays_state     the state, [12][npix^2] in the order b1 b2 t1 t2 A11 A12 A21 A22 T11 T12 T21 T22; waits for the
 *                         stream.  Before any step: the start state
 *   slicer_rays_planes    the number of steps since create / reset and the last plane's chi (either may be NULL) */
typedef struct slicer_rays *slicer_rays_handle;
#define SLICER_RAYS_KAPPA 0
#define SLICER_RAYS_GAMMA1 1
#define SLICER_RAYS_GAMMA2 2
#define SLICER_RAYS_OMEGA 3
#define SLICER_RAYS_DEFLECTION1 4
#define SLICER_RAYS_DEFLECTION2 5
#define SLICER_RAYS_COUNT 6
int slicer_rays_create(slicer_handle h, int32_t npix, double spacing, slicer_rays_handle *out);
int slicer_rays_reset(slicer_rays_handle rh);
int slicer_rays_step(slicer_rays_handle rh, double chi, const float *d_alpha1, const float *d_alpha2,
                     const float *d_kappa, const float *d_gamma1, const float *d_gamma2);
int slicer_rays_observe(slicer_rays_handle rh, double chi_s, float *const d_out[SLICER_RAYS_COUNT]);
int slicer_rays_state(slicer_rays_handle rh, double *host);
int slicer_rays_planes(slicer_rays_handle rh, int32_t *n_steps, double *chi_last);
int slicer_rays_destroy(slicer_rays_handle rh);
/* Zero the accumulators and forget the means: the handle as just created.  Enqueued, no synchronisation. */
int slicer_kappa_reset(slicer_kappa_handle kh);
/* Per-plane lensing strengths for the ray tracer, host only; the arguments, the background and the refusals of
 * slicer_lensing_weights.  strength[p] = 4 pi / (c^2/G) * g_p * (1 + zl_p) * chi(zl_p) / a_p: the lens map of plane p
 * is L_p = strength[p] (m_p - mean m_p), and Born's c_sp = strength[p] (chi_s - chi_p) / chi_s up to rounding.
 * chil[p] = chi(zl_p); chis[s] = chi(zs[s]); n_in_front[s] = the number of planes with z(ld2[p]) <= zs[s] + 1e-4 (the rule of
 * slicer_lensing_weights).  zs = NULL: the far-edge redshifts z(ld2[p]) (n_sources must equal n_planes).  chil, chis and
 * n_in_front may be NULL. */
int slicer_lensing_plane_strengths(double omega_m, double omega_lambda, double w0, double wa, double fov_deg, int32_t npix,
                                   int32_t growth, int32_t physical, int32_t n_planes, const double *ld,
                                   const double *ld2, const double *zsnap, int32_t n_sources, const double *zs,
                                   double *strength, double *chil, double *chis, int32_t *n_in_front);

/* ---- Gaussian and aperture-mass smoothing of a map ----
 * The input is any device f32 map x of npix^2 pixels (row-major), 1 <= npix <= 131072, which is only read; the output is one
 * f32 map of npix^2 pixels owned by the handle.  Scale s = sigma_pix in pixels (f64, finite, > 0), truncation t (f64,
 * 1 <= t <= 8).  Radius R = floor(t s + 0.5), the rule of scipy.ndimage.gaussian_filter, 1 <= R <= SLICER_SMOOTH_MAX_RADIUS.
 * Weights, for k = 0 ... R, in f64, each operation rounded once (RN), no FMA: q_k = RN(RN(k k) / RN(2 RN(s s))),
 * g_k = exp(-q_k) (libm's), h_k = RN(q_k g_k); g_0 = 1 and h_0 = 0.
 * Line operator L_w along one axis, for a table w, on f64 values v, samples outside 0 ... npix-1 taken as +0.0:
 *   acc_0 = RN(w_0 v[i]);  acc_k = RN(acc_{k-1} + RN(w_k RN(v[i-k] + v[i+k])))  for k = 1 ... R, from the centre outwards.
 * SLICER_SMOOTH_GAUSS: x widened exactly to f64; T = L_g along axis 1 (kept in f64); A = L_g of T along axis 0; N[i] = L_g of
 *   a line of npix ones; out[i][j] = RN32(RN(A / RN(N[i] N[j]))).  The filter does not wrap: near an edge it is renormalised
 *   by the weight that fell inside the map, so a constant map stays constant.
 * SLICER_SMOOTH_MAP: the aperture mass with U(r) = (1 - r^2 / 2 s^2) exp(-r^2 / 2 s^2) / (2 pi s^2), r in pixels (van Waerbeke
 *   1998), on the grid g x g - h x g - g x h: G = L_g and H = L_h along axis 1; D = RN(G - H); a = L_g of D and b = L_h of G
 *   along axis 0; c = RN(1 / RN(RN(RN(2 pi) s) s)); out = RN32(RN(c RN(a - b))).  Not renormalised: pixels nearer than R to an
 *   edge see a truncated aperture (crop by the radius).  The truncated, sampled filter is compensated only approximately
 *   (DESIGN.md): take t = 5 where that matters.
 * NaN and +-inf pixels propagate by IEEE through exactly the (2R+1)^2 outputs whose window holds them, clipped to the map;
 * NaN payloads and the sign of a zero result are not part of the contract.  The same input gives the same bits on every
 * run; a numpy restatement fed with slicer_smooth_weights reproduces every output value.
 *   slicer_smooth_weights     host only: the radius and the tables g, h [radius + 1] (any of the three may be NULL).
 *                             SLICER_ERR_ARG (message through slicer_last_error(NULL)): s or t not finite or out of range,
 *                             R < 1; SLICER_ERR_UNSUPPORTED: R > 128 (run a wider filter on a level of the moments pyramid)
 *   slicer_smooth_create      on the device and stream of h (h's current one: slicer_set_stream, destroy it before h).
 *                             The numbers are checked before the handle, so that they can be checked without a device:
 *                             npix < 1, an unknown kind and the refusals of slicer_smooth_weights; npix > 131072:
 *                             SLICER_ERR_UNSUPPORTED.  Device memory: 4 bytes a pixel of output, 8 (GAUSS) or 16 (MAP) of
 *                             f64 intermediate, 8 npix of N and the tables (SLICER_ERR_NOMEM)
 *   slicer_smooth_run         any device f32 map of the handle's npix^2 pixels; enqueued, no synchronisation.
 *                             SLICER_ERR_ARG: a NULL map, a map that overlaps the handle's own output (a second handle
 *                             smooths a smoothed map)
 *   slicer_smooth_run_npix    the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                             SLICER_ERR_ARG), with the N of that npix; nothing is carried over between runs
 *   slicer_smooth_device_map  the output of the last run, npix^2 floats of that run, valid until the next run or destroy
 *   slicer_smooth_read        the same to the host; waits for the stream.  Both before any run: SLICER_ERR_STATE */
typedef struct slicer_smooth *slicer_smooth_handle;
#define SLICER_SMOOTH_GAUSS 0
#define SLICER_SMOOTH_MAP 1
#define SLICER_SMOOTH_MAX_RADIUS 128
int slicer_smooth_weights(double sigma_pix, double truncate, int32_t *radius, double *g, double *h);
int slicer_smooth_create(slicer_handle h, int32_t npix, int32_t kind, double sigma_pix, double truncate,
                         slicer_smooth_handle *out);
int slicer_smooth_run(slicer_smooth_handle sh, const float *d_map);
int slicer_smooth_run_npix(slicer_smooth_handle sh, const float *d_map, int32_t npix);
int slicer_smooth_device_map(slicer_smooth_handle sh, float **d_out);
int slicer_smooth_read(slicer_smooth_handle sh, float *out);
int slicer_smooth_destroy(slicer_smooth_handle sh);

/* ---- shape noise for a map, counter-based ----
 * Generator: Philox4x32-10 (Salmon et al. 2011): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl key increments
 * 0x9E3779B9, 0xBB67AE85, ten rounds, the key bumped between rounds; a round maps (c0, c1, c2, c3) to
 * (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
 * Addressing: a map is a flat array of npix^2 f32 values, p = i npix + j; block b (u64) is the pixels 4 b ... 4 b + 3 of the
 * flat index (blocks straddle rows when 4 does not divide npix) and draws once: counter (b & 0xffffffff, b >> 32, realisation,
 * stream), key (seed & 0xffffffff, seed >> 32) -> words w0 ... w3.  The value at a pixel depends on (seed, stream,
 * realisation, p) and on nothing else.
 * Normals, all in f64: u(w) = (w + 0.5) 2^-32, exact and inside (0, 1); R_a = sqrt(-2 log u(w0)), R_b = sqrt(-2 log u(w2));
 * z0 = R_a cospi(2 u(w1)), z1 = R_a sinpi(2 u(w1)), z2 = R_b cospi(2 u(w3)), z3 = R_b sinpi(2 u(w3)); 2 u is exact, so
 * the argument reduction is; |z| <= 6.77.
 * Output: out[p] = RN32(RN64(x[p] + RN64(sigma z))), x widened exactly, no FMA; x == NULL (pure noise): RN32(RN64(sigma z)).
 * z is never rounded to f32 on its own.  The words are exact, the same bits on the host and on the device.  log and sincospi
 * are not correctly rounded, so the values carry a bound, against ref evaluated exactly from the same words:
 *   |out - ref| <= 2^-24 |ref| (1 + 2^-20) + 8 2^-53 sigma R,  R the sample's own R_a or R_b   (DESIGN.md counts the 8).
 * Bitwise: two runs are equal; both load paths; any partition of a map into run_at pieces is one run; a smaller run_npix map
 * is the first npix^2 flat values of a larger one; sigma = 0 returns x as values; NaN and +-inf in x stay in their own pixel.
 *   slicer_noise_words          host only: the four words of one block
 *   slicer_noise_sigma_pix      host only: sigma_pix = sigma_e / sqrt(n_gal A_pix), A_pix = (60 angle_deg / npix)^2 arcmin^2,
 *                               in f64 as RN(sigma_e / sqrt(RN(n_gal RN(side side)))), side = RN(RN(60 angle_deg) / npix).
 *                               sigma_e is the ellipticity dispersion PER COMPONENT (the total dispersion of both components
 *                               is sqrt(2) times it); n_gal per arcmin^2.  SLICER_ERR_ARG: a non-finite or non-positive argument
 *   slicer_smooth_noise_gain    host only: the rms of slicer_smooth_*'s output for white noise of unit variance, at a pixel at
 *                               least the radius away from every edge, in long double from slicer_smooth_weights' tables:
 *                               GAUSS sum g^2 / (sum g)^2, MAP c sqrt(sum_ij (g_i g_j - h_i g_j - g_i h_j)^2), sums over
 *                               -R ... R.  sigma_smoothed = sigma_pix gain.  Refusals: those of slicer_smooth_weights
 *   slicer_noise_create         on the device and stream of h (h's current one: slicer_set_stream, destroy it before h);
 *                               one f32 npix^2 output owned by the handle.  The numbers are checked before the handle:
 *                               npix < 1 SLICER_ERR_ARG, npix > 131072 SLICER_ERR_UNSUPPORTED
 *   slicer_noise_run            d_map: any device f32 map of the handle's npix^2 pixels, or NULL; enqueued, no synchronisation.
 *                               d_map may be the handle's own output (a second layer of noise); any other overlap with it:
 *                               SLICER_ERR_ARG.  sigma finite and >= 0 (checked before the handle)
 *   slicer_noise_run_npix       the same of a smaller map, 1 <= npix <= the handle's
 *   slicer_noise_run_at         the 1-D form the other two call: pixels first_pixel ... first_pixel + count - 1 of the flat
 *                               index, first_pixel a multiple of 4 (any u64), 1 <= count <= the handle's npix^2; d_map[0] and
 *                               the output's first value both are pixel first_pixel
 *   slicer_noise_words_device   the words of blocks first_block ... first_block + n_blocks - 1 (1 <= n_blocks <= 2^32) into the
 *                               device buffer d_out, 4 words per block
 *   slicer_noise_device_map     the output of the last run (its count of floats), valid until the next run or destroy
 *   slicer_noise_read           the same to the host; waits for the stream.  Both before any run: SLICER_ERR_STATE */
typedef struct slicer_noise *slicer_noise_handle;
int slicer_noise_words(uint64_t seed, uint32_t stream, uint32_t realisation, uint64_t block, uint32_t out[4]);
int slicer_noise_sigma_pix(double sigma_e, double ngal_arcmin2, double angle_deg, int32_t npix, double *sigma_pix);
int slicer_smooth_noise_gain(int32_t kind, double sigma_pix, double truncate, double *gain);
int slicer_noise_create(slicer_handle h, int32_t npix, uint64_t seed, slicer_noise_handle *out);
int slicer_noise_run(slicer_noise_handle nh, const float *d_map, double sigma, uint32_t stream, uint32_t realisation);
int slicer_noise_run_npix(slicer_noise_handle nh, const float *d_map, int32_t npix, double sigma, uint32_t stream,
                          uint32_t realisation);
int slicer_noise_run_at(slicer_noise_handle nh, const float *d_map, uint64_t first_pixel, uint64_t count, double sigma,
                        uint32_t stream, uint32_t realisation);
int slicer_noise_words_device(slicer_noise_handle nh, uint64_t first_block, uint64_t n_blocks, uint32_t stream,
                              uint32_t realisation, uint32_t *d_out);
int slicer_noise_device_map(slicer_noise_handle nh, float **d_out);
int slicer_noise_read(slicer_noise_handle nh, float *out);
int slicer_noise_destroy(slicer_noise_handle nh);

/* ---- Starlet transform of a map and binned absolute sums, the starlet l1-norm ----
 * The starlet is the isotropic undecimated wavelet transform with the B3-spline (a trous).  The input is any device f32 map
 * x of npix^2 pixels (row-major), 1 <= npix <= 131072, which is only read; the outputs are J + 1 f32 maps of npix^2 pixels
 * owned by the handle, 1 <= J <= SLICER_STARLET_MAX_SCALES.
 * Index rule: the map is mirrored about its edge pixels, which are not repeated.  refl(i) = 0 for npix = 1; otherwise
 * m = i mod 2 (npix - 1) taken non-negative and refl(i) = m if m < npix, else 2 (npix - 1) - m.  The rule is applied as often
 * as needed: the reach 2 * 2^j may exceed npix many times over.
 * Line operator A_d along one axis, on f64 values v, step d = 2^j, every operation one IEEE f64 operation rounded once (RN),
 * no FMA:  a = RN(v[refl(i - d)] + v[refl(i + d)]);  b = RN(v[refl(i - 2 d)] + v[refl(i + 2 d)]);
 *   out[i] = RN(RN(RN(RN(6 v[i]) + RN(4 a)) + b) * 0.0625).
 * Levels: c_0 is x widened exactly; for j = 0 ... J-1, c_{j+1} = A_d along axis 0 of (A_d along axis 1 of c_j) and
 * w_{j+1} = RN32(RN(c_j - c_{j+1})); the coarse map is RN32(c_J).  The c_j are f64 and are never rounded to f32 between
 * levels.
 * NaN and +-inf pixels propagate by IEEE; NaN payloads and the sign of a zero are not part of the contract.  The same input
 * gives the same bits on every run; a numpy restatement reproduces every output value.  It follows that a constant map has
 * coarse == the map and every w_j == 0 exactly, and that, summed in f64, |coarse + sum_j w_j - x| <=
 * 2^-24 (|coarse| + sum_j |w_j|) (1 + 2^-20) per pixel: the computed c_j telescope exactly, only the J + 1 roundings to f32
 * remain.  Out of scope: the second-generation (positive-reconstruction) starlet, decimated transforms, masks, periodic
 * boundaries.
 *   slicer_starlet_gains       host only: gain_w [scales], the rms of w_1 ... w_scales, and gain_coarse, that of the coarse
 *                              map, for white noise of unit variance at a pixel farther than the reach from every edge
 *                              (either may be NULL).  In long double from the exact integer tables H_0 = delta, H_j =
 *                              H_{j-1} * (1, 4, 6, 4, 1) / 16 dilated by 2^{j-1}: gain_j = sqrt(sum_ab (H_{j-1}[a] H_{j-1}[b] -
 *                              H_j[a] H_j[b])^2), gain_coarse = sum_a H_J[a]^2; 0.8907963, 0.2006639, 0.0855075, ...  scales
 *                              outside 1..12: SLICER_ERR_ARG (message through slicer_last_error(NULL))
 *   slicer_starlet_create      on the device and stream of h (h's current one: slicer_set_stream, destroy it before h).
 *                              The numbers are checked before the handle, so that they can be checked without a device:
 *                              npix < 1 or scales outside 1..12: SLICER_ERR_ARG; npix > 131072: SLICER_ERR_UNSUPPORTED.
 *                              Device memory: 4 (J + 1) bytes a pixel of outputs and 16 of f64 levels (SLICER_ERR_NOMEM)
 *   slicer_starlet_run         any device f32 map of the handle's npix^2 pixels; one kernel a level, enqueued, no
 *                              synchronisation.  SLICER_ERR_ARG: a NULL map, a map that overlaps the handle's own buffers
 *   slicer_starlet_run_npix    the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                              SLICER_ERR_ARG), so that one handle serves every level of a moments pyramid
 *   slicer_starlet_device_map  scale 1 ... J: w_scale of the last run; scale 0: the coarse map (others: SLICER_ERR_ARG);
 *                              npix^2 floats of that run, valid until the next run or destroy
 *   slicer_starlet_read        the same to the host; waits for the stream.  Both before any run: SLICER_ERR_STATE
 * Binned absolute sums.  The input is any device f32 map of npix^2 pixels, 1 <= npix <= 131072, which is only read; the edges
 * are those of slicer_peaks_*: f64, finite, strictly ascending, 1 <= B <= SLICER_PEAKS_MAX_BINS.  The bin of a pixel is the
 * PDF's of row N10: x widened exactly to f64 and compared in f64, the last bin closed, `below`, `above` and `nan` as there.
 * Per bin the int64 count, exact and equal to slicer_peaks_read's pdf, and the f64 sum of |x| over the bin's pixels (|x|
 * widened is exact); `below` and `above` have sums too; NaN pixels enter no sum.  The sums are accumulated in f64 over a
 * fixed partition of the map with no floating-point atomics: two runs give the same bits; the order is otherwise the
 * implementation's.  Against the exact sum S_b: |sum_b - S_b| <= count_b 2^-53 S_b (all terms are non-negative, so any order
 * of count_b - 1 additions stays inside it).
 *   slicer_l1norm_create    arguments, refusals and their order as slicer_peaks_create.  Device memory: the edges, 16 B + 40
 *                           bytes of results and at most max(64, 8 per compute unit) rows of 12 B + 28 bytes
 *   slicer_l1norm_run       any device f32 map of the handle's npix^2 pixels (e.g. slicer_starlet_device_map); enqueued, no
 *                           synchronisation.  A NULL map: SLICER_ERR_ARG
 *   slicer_l1norm_run_npix  the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others: SLICER_ERR_ARG)
 *   slicer_l1norm_read      counts, sums [B] each, below, above, the NaN count, below_sum, above_sum [1] each, of the last run
 *                           (any of them NULL); waits for the stream.  Before any run: SLICER_ERR_STATE */
typedef struct slicer_starlet *slicer_starlet_handle;
typedef struct slicer_l1norm *slicer_l1norm_handle;
#define SLICER_STARLET_MAX_SCALES 12
int slicer_starlet_gains(int32_t scales, double *gain_w, double *gain_coarse);
int slicer_starlet_create(slicer_handle h, int32_t npix, int32_t scales, slicer_starlet_handle *out);
int slicer_starlet_run(slicer_starlet_handle sh, const float *d_map);
int slicer_starlet_run_npix(slicer_starlet_handle sh, const float *d_map, int32_t npix);
int slicer_starlet_device_map(slicer_starlet_handle sh, int32_t scale, float **d_out);
int slicer_starlet_read(slicer_starlet_handle sh, int32_t scale, float *host);
int slicer_starlet_destroy(slicer_starlet_handle sh);
int slicer_l1norm_create(slicer_handle h, int32_t npix, int32_t n_edges, const double *edges, slicer_l1norm_handle *out);
int slicer_l1norm_run(slicer_l1norm_handle lh, const float *d_map);
int slicer_l1norm_run_npix(slicer_l1norm_handle lh, const float *d_map, int32_t npix);
int slicer_l1norm_read(slicer_l1norm_handle lh, int64_t *counts, double *sums, int64_t *below, int64_t *above, int64_t *n_nan,
                       double *below_sum, double *above_sum);
int slicer_l1norm_destroy(slicer_l1norm_handle lh);

/* ---- Masked pseudo-C_l: coupled bandpowers, mode-coupling matrix, decoupling ----
 * Notation of the power spectra above (row N7): n = npix, theta, the [n][n/2+1] half plane, the integer m2, the edges
 * r_0 < ... < r_B in units of l_f and their bins (the last one closed on the right).  H_b: the half-plane coefficients
 * in bin b, each one mode, N_b = |H_b|.  F_b: the FULL-plane modes (both signs of both indices) whose m2 lies in bin b,
 * m2 = 0 included when the bin holds it.  One mask w (f32, n^2 pixels, finite values) is shared by all maps:
 *   masked map          w * kappa_s, the f32 product (one rounding), taken as the transform loads the map;
 *                       khat_s = rfft2(w * kappa_s) in f64: bitwise slicer_shear_spectrum of the multiplied map under the
 *                       same shear_split
 *   coupled bandpowers  Ct_st,b = theta^2 / n^4 * (1 / N_b) * sum over H_b of Re(khat_s conj khat_t): bitwise what
 *                       slicer_power_read gives for the multiplied maps
 *   coupling matrix     M[b][b'] = 1 / (N_b n^4) * sum over k in H_b, k' in F_b' of |what(k - k')|^2, what = fft2(w)
 *                       unnormalised; w = c everywhere gives M = c^2 I.  Computed as: A = irfft2(|rfft2 w|^2), the circular
 *                       autocorrelation of the mask, in f64; per b', G = irfft2 of the indicator of F_b' in f64,
 *                       Q = Re rfft2(A G) / n^2 and M[b][b'] = (1 / N_b) * the sum of Q over H_b, summed in the order of
 *                       slicer_power_run.  Rows and columns of empty bins (N_b = 0) are 0.
 *   decoupled           Ch_st = M_act^-1 Ct_st on the active bins, those with N_b > 0; NaN in the others.  An f64 LU with
 *                       partial pivoting on the host, factorised once per mask; two substitutions per pair in
 *                       slicer_pcl_read.  Modes outside all edges are dropped as in N7: power that the mask couples to or
 *                       from them is not modelled, so the edges should span the modes that carry power.
 *   mask moments        mean(w) and mean(w^2) in f64; fixed summation order, no floating-point atomics
 *   border taper        (NaMaster's C1 apodisation, separable) on an axis x_i = min(i, n-1-i) + 0.5, t = x_i / width_pix,
 *                       f_i = 1 if t >= 1, else t - sin(2 pi t) / (2 pi); w = (float)(f[i0] * f[i1]), the product in f64;
 *                       with a user mask as well, that value times the user mask in f32
 * Out of scope: purification, contaminant deprojection, bandpower window functions, a different mask per map,
 * noise-bias subtraction, the curved sky.  Spin-2 fields and E/B are row N21 below (slicer_pcl2_*).
 *   slicer_pcl_taper     host only: f [npix] in f64.  npix < 2, or a width that is not positive and finite: SLICER_ERR_ARG
 *   slicer_pcl_create    arguments and refusals as slicer_power_create, except that the edges are required (NULL:
 *                        SLICER_ERR_ARG) and more than SLICER_PCL_MAX_BINS bins are SLICER_ERR_UNSUPPORTED.  Device memory
 *                        beyond slicer_power_create's: A, G and one spectrum in f64 and w, 3 * 8 npix^2 + 4 npix^2 bytes
 *                        (the spectrum 16 npix (npix/2+1)), and the taper table (SLICER_ERR_NOMEM)
 *   slicer_pcl_set_mask  d_mask: a device f32 npix^2 map or NULL (the taper alone); taper_width_pix: 0 for the mask alone.
 *                        Both absent, or a width that is negative or not finite: SLICER_ERR_ARG.  Builds w, the moments, A,
 *                        M and the LU, and waits for the stream.  A mask with a value that is not finite, or whose active M
 *                        has a zero or non-finite pivot (an all-zero mask is one; "coupling matrix singular"):
 *                        SLICER_ERR_ARG.  A new mask replaces the old one and invalidates the last run; after a refused
 *                        one the handle has no mask.
 *   slicer_pcl_read_mask w, npix^2 f32; slicer_pcl_coupling: M [B][B] row-major, mean(w), mean(w^2) (any of them NULL).
 *                        Before a mask: SLICER_ERR_STATE
 *   slicer_pcl_run       n_maps device f32 maps; enqueued, no synchronisation.  Before a mask: SLICER_ERR_STATE
 *   slicer_pcl_spectrum  khat of map `map` of the last run, as slicer_power_spectrum
 *   slicer_pcl_read      cl (decoupled) and coupled [pairs][B] in the pair order of slicer_power_create, ell_mean and counts
 *                        [B] (any of them NULL); waits for the stream.  Before a run: SLICER_ERR_STATE
 * No atomics: the same mask and maps give bitwise the same M and bandpowers. */
typedef struct slicer_pcl_s *slicer_pcl_handle;
#define SLICER_PCL_MAX_BINS 512
int slicer_pcl_taper(int32_t npix, double width_pix, double *f);
int slicer_pcl_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_maps, int32_t cross, int32_t n_edges,
                      const double *edges, slicer_pcl_handle *out);
int slicer_pcl_set_mask(slicer_pcl_handle ph, const float *d_mask, double taper_width_pix);
int slicer_pcl_read_mask(slicer_pcl_handle ph, float *host);
int slicer_pcl_coupling(slicer_pcl_handle ph, double *M, double *mean_w, double *mean_w2);
int slicer_pcl_run(slicer_pcl_handle ph, const float *const *d_maps);
int slicer_pcl_spectrum(slicer_pcl_handle ph, int32_t map, double *host);
int slicer_pcl_read(slicer_pcl_handle ph, double *cl, double *coupled, double *ell_mean, int64_t *counts);
int slicer_pcl_destroy(slicer_pcl_handle ph);

/* ---- E/B pseudo-C_l of masked shear maps, spin-2 ----
 * Notation of rows N7 and N17 above: n = npix, the [n][n/2+1] half plane, the integer mode indices j0 = fftfreq (-n/2 for
 * the Nyquist row of an even n) and j1 = 0 ... n/2 in the half plane (fftfreq in the full plane), m2 = j0^2 + j1^2, the
 * bins, H_b, F_b and N_b (the m2 = 0 mode stays in a bin when r_0 = 0), and one shared f32 mask w built exactly as
 * slicer_pcl_set_mask builds it (taper, user mask, or both).
 *   spin phases         for a mode with m2 > 0, every operation one IEEE f64 operation, no FMA:
 *                         c2 = (j0^2 - j1^2) / m2, s2 = 2 j0 j1 / m2 (the integers are exact),
 *                         c4 = c2 c2 - s2 s2 (each product rounded, then the difference), s4 = 2 (c2 s2);
 *                       at m2 = 0, c2 = c4 = 1 and s2 = s4 = 0: the rotation is the identity there.  On the Nyquist lines of
 *                       an even n (|j0| = n/2 or |j1| = n/2) s2 = s4 = 0 and c2, c4 keep their values: the grid cannot
 *                       tell +n/2 from -n/2, so the odd functions take the mean over the two aliases (otherwise the
 *                       sine-weighted indicators would not be Hermitian and their inverse transforms not real).  There
 *                       c2^2 + s2^2 < 1, so E and B are NOT separated on those lines; edges that stop below n/2 avoid them.
 *                       (C_s, S_s) = (c2, s2) for s = 2 and (c4, s4) for s = 4.
 *   E/B spectra         of a field (gamma1, gamma2): g1 = rfft2(w gamma1), g2 = rfft2(w gamma2), bitwise row N17's masked
 *                       transforms; Ehat = c2 g1 + s2 g2, Bhat = c2 g2 - s2 g1 on the real and imaginary parts separately,
 *                       each product rounded, then the sum.  This inverts row N6's filters (axis 0 is the slow axis).  With
 *                       with_kappa the field's third component is khat = rfft2(w kappa), bitwise row N17's.
 *   component list      per field E, B, and kappa if present; field f's components are 3f, 3f+1, 3f+2 (2f, 2f+1 without kappa)
 *   coupled bandpowers  Ct_xy,b = theta^2 / n^4 * (1 / N_b) * sum over H_b of Re(x conj y): slicer_power_run's slices,
 *                       summation order and finish on those spectra, no atomics
 *   coupling matrices   for s = 2, 4, what = fft2(w) unnormalised:
 *                         M_s[b][b'] = 1 / (N_b n^4) * sum over k in H_b, k' in F_b' of |what(k - k')|^2 *
 *                                      (C_s(k) C_s(k') + S_s(k) S_s(k'))      (the weight cos s(phi' - phi))
 *                         X_s[b][b'] = the same sum with (C_s(k) S_s(k') - S_s(k) C_s(k'))  (sin s(phi' - phi); zero for a
 *                                      mirror-symmetric mask, not in general)
 *                       and M_0 is row N17's M, bitwise.  Computed per non-empty b' with A = irfft2(|rfft2 w|^2):
 *                       G_c = irfft2(1[F_b'] C_s), G_s = irfft2(1[F_b'] S_s), Q_c = Re rfft2(A G_c) / n^2,
 *                       Q_s = Re rfft2(A G_s) / n^2, M_s[.][b'] = the binned mean over H_b of C_s(k) Q_c + S_s(k) Q_s and
 *                       X_s[.][b'] that of C_s(k) Q_s - S_s(k) Q_c.  Rows and columns of empty bins are 0.  Five inverse and
 *                       five forward transforms per non-empty bin, against row N17's one and one.
 *   decoupling          the mask's first-order mixing, spectra taken flat within a bin as in row N17:
 *                         kappa kappa:                 Ct = M_0 C
 *                         (kE, kB) of a field pair:    the 2B x 2B system [[M_2, -X_2], [X_2, M_2]]
 *                         (EE, EB, BE, BB) of a pair (f, g), EB = E_f B_g and BE = B_f E_g: the 4B x 4B system
 *                             [ P -T -T  R ]
 *                             [ T  P -R -T ]     P = (M_0 + M_4) / 2, R = (M_0 - M_4) / 2, T = X_4 / 2
 *                             [ T -R  P -T ]
 *                             [ R  T  T  P ]
 *                         (for f = g, BE is EB).  Each system is restricted to the active bins (N_b > 0), factorised once per
 *                       mask by row N17's f64 LU with partial pivoting on the host and solved per pair in slicer_pcl2_read; the
 *                       other bins read NaN.  Because the 4B system is solved on the host, at most SLICER_PCL2_MAX_BINS bins.
 * Out of scope: purification, bandpower window functions, per-field masks, noise bias, the curved sky, spin-1, and the
 * driver reading --raytrace outputs (slicer_pcl2_run takes any device maps, the ray tracer's included).
 *   slicer_pcl2_phases    host only: C, S [npix][npix/2+1] in f64 for spin 2 or 4.  Another spin, npix < 2 or a null
 *                         output: SLICER_ERR_ARG
 *   slicer_pcl2_create    n_fields fields of (gamma1, gamma2) and, with with_kappa = 1, kappa.  cross = 0: the pairs within
 *                         each field, field after field, in slicer_power_create's pair order over (E, B, kappa):
 *                         EE, EB, Ek, BB, Bk, kk (EE, EB, BB without kappa).  cross = 1: all pairs i <= j of the component
 *                         list in slicer_power_create's pair order.  Refusals as slicer_pcl_create; more than
 *                         SLICER_PCL2_MAX_BINS bins, or n_fields outside 1 ... 128 / (2 + with_kappa) (the power handle's
 *                         128 maps): SLICER_ERR_UNSUPPORTED; with_kappa or cross not 0 or 1: SLICER_ERR_ARG.  Device memory
 *                         beyond slicer_power_create's over the components: A, G_c, G_s (8 npix^2 each), w (4 npix^2) and
 *                         four spectra of 16 npix (npix/2+1) bytes (SLICER_ERR_NOMEM)
 *   slicer_pcl2_set_mask  as slicer_pcl_set_mask; "coupling matrix singular" (SLICER_ERR_ARG) for a zero or non-finite pivot
 *                         in any of the three systems.  A new mask invalidates the last run; after a refused one the handle
 *                         has no mask.  Waits for the stream
 *   slicer_pcl2_read_mask w; slicer_pcl2_coupling: M_0, M_2, X_2, M_4, X_4 [B][B] row-major, mean(w), mean(w^2) (any of
 *                         them NULL).  Before a mask: SLICER_ERR_STATE
 *   slicer_pcl2_run       the device f32 maps, per field gamma1, gamma2, then kappa with with_kappa; enqueued, no
 *                         synchronisation.  Before a mask: SLICER_ERR_STATE
 *   slicer_pcl2_spectrum  the spectrum of component comp (0, 1, 2 = E, B, kappa) of field `field` of the last run; auto mode
 *                         keeps the last field's only (SLICER_ERR_STATE for another)
 *   slicer_pcl2_read      cl (decoupled) and coupled [pairs][B] in the order above, ell_mean and counts [B] (any of them
 *                         NULL); waits for the stream.  Before a run: SLICER_ERR_STATE
 * No atomics: the same mask and maps give bitwise the same matrices and bandpowers. */
typedef struct slicer_pcl2_s *slicer_pcl2_handle;
#define SLICER_PCL2_MAX_BINS 128
int slicer_pcl2_phases(int32_t npix, int32_t spin, double *C, double *S);
int slicer_pcl2_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_fields, int32_t with_kappa,
                       int32_t cross, int32_t n_edges, const double *edges, slicer_pcl2_handle *out);
int slicer_pcl2_set_mask(slicer_pcl2_handle ph, const float *d_mask, double taper_width_pix);
int slicer_pcl2_read_mask(slicer_pcl2_handle ph, float *host);
int slicer_pcl2_coupling(slicer_pcl2_handle ph, double *M0, double *M2, double *X2, double *M4, double *X4,
                         double *mean_w, double *mean_w2);
int slicer_pcl2_run(slicer_pcl2_handle ph, const float *const *d_maps);
int slicer_pcl2_spectrum(slicer_pcl2_handle ph, int32_t field, int32_t comp, double *host);
int slicer_pcl2_read(slicer_pcl2_handle ph, double *cl, double *coupled, double *ell_mean, int64_t *counts);
int slicer_pcl2_destroy(slicer_pcl2_handle ph);

/* ---- Real-space two-point correlation functions xi_kk(theta), xi+(theta), xi-(theta) ----
 * Fields and weights.  A spin-0 field is one f32 map a; a spin-2 field is two, (a1, a2) = (gamma1, gamma2).  Every map is
 * n^2 = npix^2 pixels, row-major, axis 0 slow and component 1 (row N6's convention), 2 <= npix <= 16383, and is only read.
 * A field value that is not finite is the caller's, as in row N7.  One optional f32 weight map w is shared by all fields
 * (NULL: w = 1); it must be finite and >= 0.  The working fields are a~ = a * w, the product of the two f32 values taken
 * in f64, which is exact (row N17 takes an f32 product instead).
 * Pairs.  For a lag r = (dx, dy) != 0 along (axis 0, axis 1), |dx|, |dy| <= n - 1: C_ab(r) = sum over x of a~(x) b~(x + r),
 * over the x for which both pixels lie inside the map.  Nothing wraps.  W(r) = sum over x of w(x) w(x + r), and
 * N(r) = (n - |dx|) (n - |dy|): ordered pairs, a bin sums both signs of r.
 * Bins.  Edges in pixels, f64, finite, 0 <= r_0 < ... < r_B <= sqrt(2) (n - 1) (the f64 product of sqrt(2.0) and n - 1),
 * 1 <= B <= SLICER_XI_MAX_BINS.  A lag is in bin b iff RN64(r_b^2) <= m2 < RN64(r_{b+1}^2) on the exact integer
 * m2 = dx^2 + dy^2; the last bin is closed on the right (row N7's rule); m2 = 0 is in no bin.  L = min(ceil(r_B), n - 1) is
 * the largest |dx| or |dy| that can occur.
 * Per bin, with M_b the number of its lags:  counts = N_b = sum N(r), int64, exact, independent of w;  W_b = sum W(r) in
 * f64;  r_mean = sum W(r) sqrt(m2) / W_b.  With w = NULL, W(r) = N(r): W_b = (double)N_b and the radius sum come from the
 * integers on the host (long double), no transform.
 *   spin 0, fields a <= b   xi_ab = sum C_ab(r) / W_b  (auto: a = b only; cross: every pair, in row N7's pair order)
 *   spin 2                  xi+ = sum (C_11 + C_22) / W_b,  xi- = sum [(C_11 - C_22) c4 + (C_12 + C_21) s4] / W_b,
 *                           c4 = (dx^4 - 6 dx^2 dy^2 + dy^4) / m2^2, s4 = 4 dx dy (dx^2 - dy^2) / m2^2, from the integer lags
 *                           in f64: xi+- = <gt gt> +- <gx gx> with gt + i gx = -gamma e^(-2 i phi), phi = atan2(dy, dx),
 *                           the sign under which gt > 0 around a point mass with row N6's gamma.  For a cross pair the
 *                           first index of each C is field a's component, the second field b's.
 * A bin is empty when M_b = 0 or W_b <= 2^-30 sum w^2: its xi, xi- and r_mean are NaN, W_b and counts are still reported.
 * (Under a 0/1 mask any bin with one real pair has W_b >= 1 > 2^-30 sum w^2 for n <= 8192; one without has pure round-off.)
 * Route.  P = the smallest size >= n + L with prime factors 2, 3, 5, 7 only (slicer_shear_supported); none up to 16384:
 * SLICER_ERR_UNSUPPORTED.  n itself need not be such a size.  (1) each map is zero-padded to P^2 in f64 and transformed as
 * the f64 product with the padded weights (the r2c transform of row N6, under the shear_split option of h at create);
 * (2) one pointwise kernel forms the real spectrum: Re(conj fa fb) (spin 0, and |what|^2 for the weights),
 * Re(conj f1a f1b + conj f2a f2b) (xi+), the same with a minus sign and Re(conj f1a f2b + conj f2a f1b) (xi-);
 * (3) each spectrum is inverted in f64, every mode kept; a lag (dx, dy) sits at (dx mod P, dy mod P), and since
 * P >= n + L no lag <= L aliases; (4) the binning kernel walks the FULL window |dx|, |dy| <= L, both signs of both lags
 * (nothing is doubled), applies c4 and s4, and reduces per bin without floating-point atomics: per-workgroup partials in a
 * fixed tree, summed in a fixed order.  The same inputs give the same bits.  Every spectrum is real, so each inverse is the
 * part of its correlation that is even in r: for a cross pair slicer_xi_correlation returns (C_ab(r) + C_ab(-r)) / 2
 * where C_ab itself is not even; the bins, which hold both signs, do not see the difference.
 * Out of scope: kappa-gamma_t (galaxy-galaxy lensing) and the parity-odd xi_x, per-field weights, shear shape noise, COSEBIs
 * and band powers from xi, the curved sky, lags beyond P = 16384.
 *   slicer_xi_bins         host only: counts N_b and lags M_b [B] by enumeration, and P (any of them NULL).  Refusals as
 *                          slicer_xi_create's of npix and the edges (message through slicer_last_error(NULL))
 *   slicer_xi_create       on the device and stream of h.  spin: 0 or 2 (others: SLICER_ERR_ARG); 1 <= n_fields <= 32 (below:
 *                          SLICER_ERR_ARG, above: SLICER_ERR_UNSUPPORTED); cross: 0 or 1 (SLICER_ERR_ARG).  npix < 2, edges that
 *                          are NULL, fewer than 2, not finite, negative, not strictly ascending or beyond sqrt(2) (npix - 1):
 *                          SLICER_ERR_ARG; npix > 16383, more than SLICER_XI_MAX_BINS bins, no P: SLICER_ERR_UNSUPPORTED.
 *                          Device memory: the plan of P, 24 P^2 bytes, 16 P (P/2+1) bytes for one spectrum and as much per
 *                          kept field component (all of them with cross, one field's without), two windows of 8 (2L+1)^2
 *                          (SLICER_ERR_NOMEM).  The handle starts with w = NULL
 *   slicer_xi_set_weights  a device f32 npix^2 map, or NULL.  Checks the values on the device, computes W(r), W_b and the
 *                          radius sums once, and waits for the stream.  A value that is negative or not finite:
 *                          SLICER_ERR_ARG, and the handle then refuses to run (SLICER_ERR_STATE) until weights are accepted.
 *                          New weights invalidate the last run
 *   slicer_xi_run          n_fields (spin 0) or 2 n_fields (spin 2: gamma1, gamma2 of field 0, then of field 1, ...) device
 *                          f32 maps; enqueued, no synchronisation.  A NULL map: SLICER_ERR_ARG
 *   slicer_xi_read         xi (spin 2: xi+) and xim (xi-; NULL for spin 0, else SLICER_ERR_ARG) [pairs][B] in the pair order
 *                          of slicer_power_create, r_mean, weights (W_b) and counts [B] (any of them NULL); waits for the
 *                          stream.  Before a run: SLICER_ERR_STATE
 *   slicer_xi_correlation  the (2L+1)^2 f64 lag window of one inverse of pair `pair` of the last run, [dx + L][dy + L]:
 *                          which = SLICER_XI_PLUS (C_ab of spin 0; C_11 + C_22), SLICER_XI_MINUS (C_11 - C_22) or
 *                          SLICER_XI_CROSS (C_12 + C_21), the latter two for spin 2 only; recomputed from the kept
 *                          transforms (auto mode keeps only the last field's: SLICER_ERR_STATE for the others).
 *                          SLICER_XI_WEIGHTS: W(r) of the weights in use, whatever `pair`, also before a run */
typedef struct slicer_xi_s *slicer_xi_handle;
#define SLICER_XI_MAX_BINS 512
#define SLICER_XI_PLUS 0
#define SLICER_XI_MINUS 1
#define SLICER_XI_CROSS 2
#define SLICER_XI_WEIGHTS 3
int slicer_xi_bins(int32_t npix, int32_t n_edges, const double *edges, int64_t *counts, int64_t *lags, int32_t *padded);
int slicer_xi_create(slicer_handle h, int32_t npix, int32_t spin, int32_t n_fields, int32_t cross, int32_t n_edges,
                     const double *edges, slicer_xi_handle *out);
int slicer_xi_set_weights(slicer_xi_handle xh, const float *d_w);
int slicer_xi_run(slicer_xi_handle xh, const float *const *d_maps);
int slicer_xi_read(slicer_xi_handle xh, double *xi, double *xim, double *r_mean, double *weights, int64_t *counts);
int slicer_xi_correlation(slicer_xi_handle xh, int32_t pair, int32_t which, double *host);
int slicer_xi_destroy(slicer_xi_handle xh);

/* ---- Betti numbers of a map's excursion sets, as exact counts ----
 * Input, thresholds, rank and excursion sets are those of the Minkowski functionals above (row N14): any device f32 map of
 * npix^2 pixels (row-major), only read; f64 thresholds t_0 < ... < t_{T-1}, finite and strictly ascending,
 * 1 <= T <= SLICER_BETTI_MAX_THRESHOLDS; k(x) = the number of t_j <= (double)x, compared in f64, k(NaN) = k(-inf) = 0,
 * k(+inf) = T; pixel x is in Q_j iff k(x) > j; positions outside the map are in no set and the field does not wrap.
 * Per threshold j = 0 ... T-1, all int64:
 *   components[j]  beta_0: the 8-connected components of Q_j; two pixels of Q_j are joined iff they share a side or a
 *                  corner
 *   holes[j]       beta_1: the 4-connected components (sides only) of the complement {pixels of the map with k <= j, NaN
 *                  pixels included} that contain no pixel of the map's first or last row or column; a complement
 *                  component that touches the rim reaches outside and is not a hole
 *   faces[j]       the pixels with k > j: the number slicer_minkowski_read gives, for cross-checks without a second handle
 *   n_nan          the NaN pixels of the last run
 * These connectivities are the ones the closed pixel complex of row N14 implies: components[j] - holes[j] equals its
 * vertices[j] - edges[j] + faces[j] exactly, on every map.  The counts are exact and the same on every run, although the
 * order in which the device unites pixels is not.
 *   slicer_betti_create    on the device and stream of h (h's current one: slicer_set_stream, destroy it before h).
 *                          The numbers are checked before the handle, so that they can be checked without a device:
 *                          npix < 1, fewer than 1 or more than 1025 thresholds, a threshold that is not finite,
 *                          thresholds not strictly ascending: SLICER_ERR_ARG; npix > SLICER_BETTI_MAX_NPIX (node ids and
 *                          npix^2 + 1 stay well inside 32 bits): SLICER_ERR_UNSUPPORTED.  Device memory: a u16 rank map
 *                          (2 npix^2 bytes), a u32 parent array of npix^2 + 1 nodes, the thresholds, at most max(64, 8 per
 *                          compute unit) rows of 4 (T + 2) bytes of counters, 8 (T + 1) bytes of link counters and
 *                          8 (T + 2) + 8 (3 T + 1) bytes of sums and results: about 6 GB at npix = 32768
 *                          (SLICER_ERR_NOMEM)
 *   slicer_betti_run       any device f32 map of the handle's npix^2 pixels (e.g. slicer_kappa_device_map); enqueued, no
 *                          synchronisation.  A NULL map: SLICER_ERR_ARG
 *   slicer_betti_run_npix  the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                          SLICER_ERR_ARG), so that one handle serves every level of a moments pyramid
 *   slicer_betti_read      components, holes, faces [T] each and the NaN count of the last run (any of them NULL); waits
 *                          for the stream.  Before any run: SLICER_ERR_STATE */
typedef struct slicer_betti *slicer_betti_handle;
#define SLICER_BETTI_MAX_THRESHOLDS 1025
#define SLICER_BETTI_MAX_NPIX 32768
int slicer_betti_create(slicer_handle h, int32_t npix, int32_t n_thresholds, const double *thresholds,
                        slicer_betti_handle *out);
int slicer_betti_run(slicer_betti_handle bh, const float *d_map);
int slicer_betti_run_npix(slicer_betti_handle bh, const float *d_map, int32_t npix);
int slicer_betti_read(slicer_betti_handle bh, int64_t *components, int64_t *holes, int64_t *faces, int64_t *n_nan);
int slicer_betti_destroy(slicer_betti_handle bh);

/* ---- Wavelet scattering coefficients of a kappa map, orders 0, 1 and 2 ----
 * Input: one device f32 map of npix^2 pixels, axis 0 slow = component 1, axis 1 contiguous = component 2 (row N6's
 * convention), only read, treated as periodic (as rows N7 and N15).  n = npix must be a size the f64 transform plans
 * (slicer_shear_supported: prime factors 2, 3, 5, 7 only, <= 16384); 1 <= J <= SLICER_SCATTERING_MAX_J scales with
 * 2^J <= n, 1 <= L <= SLICER_SCATTERING_MAX_L orientations.
 * Filter bank: Morlet filters defined in Fourier space, where they are real.  For scale j = 0 ... J-1 and orientation
 * l = 0 ... L-1: sigma = 0.8 2^j, xi = (3 pi / 4) 2^-j, s = 4 / L, theta = pi l / L (cos theta and sin theta computed on
 * the host in f64).  For an angular frequency (w1, w2) along (axis 0, axis 1):
 *   p = w1 cos theta + w2 sin theta,  q = -w1 sin theta + w2 cos theta,
 *   A(w) = exp(-sigma^2 / 2 ((p - xi)^2 + q^2 / s^2)),  B(w) = exp(-sigma^2 / 2 (p^2 + q^2 / s^2)),
 *   A^(w) = sum_m A(w + 2 pi m),  B^(w) = sum_m B(w + 2 pi m) over the nine m in {-1, 0, 1}^2, m1 outer, m2 inner, each
 *   from -1 up;  beta = A^(0) / B^(0), on the host.
 * For the mode index (a, b), 0 <= a, b < n: the signed index a_s = a for a < (n + 1) / 2 (integer division), else a - n
 * (n / 2 maps to -n / 2), w = 2 pi (a_s, b_s) / n, and psi^_{jl}[a][b] = A^(w) - beta B^(w), psi^_{jl}[0][0] = 0 exactly.
 * All of it in f64, no contraction into fused multiply-adds.
 * Transform: for a real f64 field f with fhat = rfft2(f), W_{jl} f = |ifft2(fhat_full psi^_{jl})|, the modulus of a
 * complex field.  Route (the library has no complex transform): with E[a][b] = (psi^[a][b] + psi^[(-a) mod n][(-b) mod n]) / 2
 * and O the same with a minus sign (0 at the self-conjugate modes by construction), x = irfft2(fhat E),
 * y = irfft2(-i fhat O), u = sqrt(x x + y y), rounded after each operation.
 * Outputs, all f64:
 *   s0[2]           the mean of kappa and the mean of kappa^2
 *   s1[J][L]        the mean of u1 = W_{jl} kappa
 *   p1[J][L]        the mean of u1^2: the wavelet power that s2 / s1 ratios and scattering covariances need
 *   s2[J][L][J][L]  the mean of W_{j2 l2} u1 for j2 > j1, indexed [j1][l1][j2][l2]; NaN where j2 <= j1
 * Nothing is subsampled: every field keeps n^2 pixels.  No floating-point atomics; every sum is blocked in a fixed order
 * (64 values, the blocks of a chunk, a lane butterfly, the chunks in index order, as row N15): the same input gives the
 * same bits run after run, and so does an input pointer one float off the 16-byte grid.  The coefficients are this
 * definition's; they are not pinned against any other package's filter bank.
 * Out of scope: subsampled or band-limited second-order transforms (psi^_{j2} occupies about 4^-j2 of the plane: the next
 * step), a complex transform, orders above 2, j2 <= j1, scattering covariances and phase harmonics, non-periodic edges
 * and masks, sizes that are not 2-3-5-7, plane maps.
 *   slicer_scattering_filter   host only, no device: psi^_{jl} [npix][npix] by the definition above.  Refusals as
 *                              slicer_scattering_create's of the numbers, (j, l) outside the bank and a NULL out:
 *                              SLICER_ERR_ARG (messages through slicer_last_error(NULL))
 *   slicer_scattering_create   on the device and stream of h, under the shear_split option of h at create.  The numbers are
 *                              checked before the handle and before any allocation: an npix the transform does not plan,
 *                              J > 12, L > 16: SLICER_ERR_UNSUPPORTED; J < 1, L < 1, 2^J > npix, null pointers:
 *                              SLICER_ERR_ARG.  Device memory: two spectra (khat, u1hat) and two products (fhat E,
 *                              -i fhat O) of 16 n (n/2+1) bytes each, two f64 maps x and y (16 n^2 bytes together), the
 *                              transform's buffers (16 n (n/2+1) bytes per pass of its longer chain, at most three, and
 *                              the twiddles), the partial sums (at most 64 KiB) and the results: about 48 n^2 bytes, 0.8 GB
 *                              at 4096^2 and 13 GB at 16384^2 (computed, not measured) (SLICER_ERR_NOMEM)
 *   slicer_scattering_run      any device f32 map of npix^2 pixels; enqueued, no synchronisation; every result word is
 *                              rewritten.  A NULL map: SLICER_ERR_ARG.  J L (1 + (J - 1) L / 2) pairs of f64 inverses
 *   slicer_scattering_read     s0, s1, p1, s2 of the last run (any of them NULL); waits for the stream.  Before any run:
 *                              SLICER_ERR_STATE
 *   slicer_scattering_modulus  the npix^2 f64 field u1 = W_{j1 l1} kappa (j2 = l2 = -1) or W_{j2 l2} u1 (j1 < j2 < J),
 *                              recomputed from d_map into host memory; waits for the stream; the results of the last run
 *                              stay readable.  Indices outside the bank: SLICER_ERR_ARG */
typedef struct slicer_scattering_s *slicer_scattering_handle;
#define SLICER_SCATTERING_MAX_J 12
#define SLICER_SCATTERING_MAX_L 16
int slicer_scattering_filter(int32_t npix, int32_t J, int32_t L, int32_t j, int32_t l, double *out);
int slicer_scattering_create(slicer_handle h, int32_t npix, int32_t J, int32_t L, slicer_scattering_handle *out);
int slicer_scattering_run(slicer_scattering_handle sh, const float *d_map);
int slicer_scattering_read(slicer_scattering_handle sh, double *s0, double *s1, double *p1, double *s2);
int slicer_scattering_modulus(slicer_scattering_handle sh, const float *d_map, int32_t j1, int32_t l1, int32_t j2,
                              int32_t l2, double *host);
int slicer_scattering_destroy(slicer_scattering_handle sh);

/* ---- Catalogue of a map's peaks and minima: positions, heights, sub-pixel offsets ----
 * Input: any device f32 map of npix^2 pixels (row-major), only read, 1 <= npix <= SLICER_CATALOGUE_MAX_NPIX.
 * Candidates and definition are those of slicer_peaks_* (row N10): the pixels (i, j) with 1 <= i, j <= npix-2; a peak is
 * strictly greater, in f32, than each of its 8 neighbours, a minimum strictly less; ties give neither, every comparison
 * with a NaN is false, nothing wraps.
 * Selection, given with every run: `kinds` is a bitmask, SLICER_CATALOGUE_PEAKS | SLICER_CATALOGUE_MINIMA; a peak is kept
 * iff (double)x >= min_peak, a minimum iff (double)x <= max_minimum, compared in f64 against the f64 thresholds;
 * -inf / +inf keep every one.
 * Record: slicer_catalogue_record, 32 bytes: row, col; value, the pixel itself; flags, bit 0 (SLICER_CATALOGUE_MINIMUM)
 * set for a minimum, bit 1 (SLICER_CATALOGUE_FALLBACK) where the refinement was not accepted; dy, dx, the offset of the
 * extremum from the pixel's centre along the rows and along the columns, in pixels.
 * Order: ascending row * npix + col, peaks and minima interleaved in that one order.  The order and every byte of every
 * record depend on the map and the selection alone: not on the launch shape, the number of compute units or the
 * alignment of the map, and they are the same on every run.
 * Refinement: the least-squares quadratic of the 3 x 3 window z[a][b], a the row offset and b the column offset, each in
 * {-1, 0, 1}.  Every value is widened exactly to f64; every operation is rounded once, none is fused, in this order:
 *   R(a) = (z[a][-1] + z[a][0]) + z[a][1],  C(b) = (z[-1][b] + z[0][b]) + z[1][b]
 *   gy = (R(1) - R(-1)) / 6,  gx = (C(1) - C(-1)) / 6
 *   hyy = ((R(1) + R(-1)) - 2 R(0)) / 3,  hxx = ((C(1) + C(-1)) - 2 C(0)) / 3
 *   hxy = ((z[1][1] + z[-1][-1]) - (z[1][-1] + z[-1][1])) / 4
 *   det = hyy hxx - hxy hxy
 *   dy = -((hxx gy - hxy gx) / det),  dx = -((hyy gx - hxy gy) / det)
 * The offsets are accepted iff det > 0, hyy < 0 for a peak (hyy > 0 for a minimum), dy and dx are finite, |dy| <= 0.5
 * and |dx| <= 0.5.  Otherwise dy = dx = +0.0 and SLICER_CATALOGUE_FALLBACK is set; a window with an infinite value ends
 * there.
 * Capacity: a handle holds `capacity` records, 1 <= capacity <= SLICER_CATALOGUE_MAX_CAPACITY = 2^29 (no two peaks and
 * no two minima are adjacent: at most npix^2 / 2 records, 2^29 at the largest npix).  A run always gives the exact
 * totals of the kept peaks and the kept minima and stores the first min(total, capacity) records of the order above;
 * an overflow is no error -- the counts show it -- and nothing behind `capacity` records is ever written.
 * No atomics and no waiting between workgroups; every count and total is rewritten by every run.
 * Out of scope: stacked profiles and sampling of companion maps at the records, sorting by height or a top-K on the
 * device, plateaux, periodic maps, the curved sky, FITS binary tables, npix above 32768.
 *   slicer_catalogue_create    on the device and stream of h (h's current one: slicer_set_stream, destroy it before h).
 *                              d_records: NULL, and the handle allocates its records, or a device buffer of the caller's
 *                              for `capacity` records, which must outlive the handle.  Checked before the handle, in this
 *                              order, so that they can be checked without a device: npix < 1: SLICER_ERR_ARG; npix >
 *                              SLICER_CATALOGUE_MAX_NPIX: SLICER_ERR_UNSUPPORTED; a capacity outside 1 ... 2^29, records
 *                              off the 16-byte grid, then a NULL h or out: SLICER_ERR_ARG.  Device memory: 32 bytes per
 *                              record of the capacity (unless they are the caller's), 4 bytes per segment of 64 columns of
 *                              a row -- 4 npix ceil(npix / 64) bytes: 1 MiB at 4096^2, 64 MiB at 32768^2 -- 12 bytes per 4096
 *                              segments and 24 bytes of totals (SLICER_ERR_NOMEM)
 *   slicer_catalogue_run       any device f32 map of the handle's npix^2 pixels (e.g. slicer_kappa_device_map); enqueued,
 *                              no synchronisation.  Checked in this order, the first two before the handle: kinds outside
 *                              1 ... 3, a NaN threshold, a NULL handle or map: SLICER_ERR_ARG
 *   slicer_catalogue_run_npix  the same of a smaller map of npix^2 pixels, 1 <= npix <= the handle's (others:
 *                              SLICER_ERR_ARG, after the checks above), so that one handle serves every level of a
 *                              moments pyramid (slicer_moments_device_map)
 *   slicer_catalogue_count     the kept peaks, the kept minima and the stored records of the last run (any of them NULL);
 *                              waits for the stream.  Before any run: SLICER_ERR_STATE
 *   slicer_catalogue_read      the first min(stored, max_records) records into host memory, *copied (may be NULL) their
 *                              number; waits for the stream.  Before any run: SLICER_ERR_STATE
 *   slicer_catalogue_device    where the last run left its results on the device: the records, and three int64 {peaks,
 *                              minima, stored}; ordered after the run on the handle's stream, valid until the next run or
 *                              the destroy.  Before any run: SLICER_ERR_STATE */
typedef struct slicer_catalogue *slicer_catalogue_handle;
#define SLICER_CATALOGUE_MAX_NPIX 32768
#define SLICER_CATALOGUE_MAX_CAPACITY 536870912 /* 2^29 */
#define SLICER_CATALOGUE_PEAKS 1    /* kinds */
#define SLICER_CATALOGUE_MINIMA 2
#define SLICER_CATALOGUE_MINIMUM 1u  /* flags */
#define SLICER_CATALOGUE_FALLBACK 2u
typedef struct {
    int32_t row, col;
    float value;
    uint32_t flags;
    double dy, dx;
} slicer_catalogue_record;
int slicer_catalogue_create(slicer_handle h, int32_t npix, int64_t capacity, void *d_records, slicer_catalogue_handle *out);
int slicer_catalogue_run(slicer_catalogue_handle ch, const float *d_map, int32_t kinds, double min_peak, double max_minimum);
int slicer_catalogue_run_npix(slicer_catalogue_handle ch, const float *d_map, int32_t kinds, double min_peak,
                              double max_minimum, int32_t npix);
int slicer_catalogue_count(slicer_catalogue_handle ch, int64_t *n_peaks, int64_t *n_minima, int64_t *stored);
int slicer_catalogue_read(slicer_catalogue_handle ch, slicer_catalogue_record *records, int64_t max_records, int64_t *copied);
int slicer_catalogue_device(slicer_catalogue_handle ch, slicer_catalogue_record **d_records, int64_t **d_counts);
int slicer_catalogue_destroy(slicer_catalogue_handle ch);

/* per-kernel HIP-event timing (off by default; adds two event records per launch) */
int slicer_profile_enable(slicer_handle h, int on);
int slicer_profile_reset(slicer_handle h);
int slicer_profile_get(slicer_handle h, slicer_kernel_time *out, int capacity, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* SLICER_AMD_H */
