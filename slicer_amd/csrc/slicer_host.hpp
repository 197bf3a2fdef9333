// slicer_host.hpp -- internal (not installed, not exported): the host layer under the C ABI of include/slicer_amd.h.
// The handle, its error and profiling plumbing, what the sub-handles (kappa, shear, FFT plan, power, moments, peaks,
// rays, smooth, noise, minkowski, bispectrum, starlet, l1norm, pcl, pcl2, xi, betti, scattering, catalogue) share, and the functions that cross the
// files of the core pass:
//   slicer_host.cpp    errors, grow-only buffers, profiling, the sub-handle helpers: SubHandle (the base of every
//                      sub-handle struct) with sub_new / sub_done for its *_create, sub_stream for its launches, sub_read
//                      for its read-backs and sub_destroy; npix_in_range and ranges_overlap for the argument checks
//   slicer_capi.cpp    entry points of the core pass
//   pass_plan.cpp      pass parameters, tile geometry, the exhaustive sweeps, slicer_debug_*
//   binned_pass.cpp    map clearing, workspaces and pending lists of the binned pipeline, the per-chunk deposit
//   thinning.cpp       shot-noise thinning and libc's rand() stream
//   reduce_meta.cpp    what ranks exchange before a cross-rank sum
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/slicer_amd.h"
#include "slicer_kernels.hpp"

#pragma GCC visibility push(hidden)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct PlaneBufs {
    DevBuf tot;
    DevBuf toti[6];
    DevBuf acc[6];  // F64/FIXED accumulators, or NGP per-file scratch
    DevBuf acc_shared;
};

struct ProfEntry {
    int name;
    hipEvent_t e0, e1;
};

// kernels as slicer_profile_get names them (kKernelNames, slicer_host.cpp)
enum {
    KN_DIRECT = 0, KN_FINALIZE, KN_FOLD, KN_SYNTH, KN_PROJECT, KN_SCAN, KN_SCATTER, KN_TILE, KN_DEBUG, KN_SORT2,
    KN_POWER_FFT, KN_POWER_BIN, KN_MOMENTS_SUM, KN_MOMENTS, KN_PEAKS, KN_PEAKS_FINISH, KN_RAYS_STEP,
    KN_RAYS_OBSERVE, KN_SMOOTH_ROWS, KN_SMOOTH_NORM, KN_SMOOTH_COLS, KN_NOISE_ADD,
    KN_NOISE_WORDS, KN_MINKOWSKI, KN_MINKOWSKI_FINISH, KN_BISPECTRUM_FFT, KN_BISPECTRUM_BAND, KN_BISPECTRUM,
    KN_BISPECTRUM_FINISH, KN_STARLET_FIRST, KN_STARLET_LEVEL, KN_STARLET_LAST, KN_L1NORM, KN_L1NORM_FINISH,
    KN_BETTI_RANK, KN_BETTI_LINK, KN_BETTI_FINISH, KN_SCATTERING_FIRST, KN_SCATTERING_SECOND, KN_COUNT
};

// Tuning and test knobs of one handle.  Read from the environment ONCE, in slicer_create (so that the tools/ scripts
// keep working), and changed per handle through slicer_set_option -- never getenv on a launch path: the per-GPU host
// threads of SLICER_amd --devices run concurrently.
struct Options {
    int k4_int = 1;       // integer tile cells: 0 never, 1 when a launch has >= 2048 particles per bin, 2 always
    int tile_log2 = 0;    // log2 tile width (0 = automatic); tile_h_log2 likewise for the height (0 = tile_log2)
    int tile_h_log2 = 0;
    int bin_batch = 0;    // particles per project+bin workgroup (0 = automatic)
    int unit_rows = 0;    // tile rows per unit (0 = automatic): band units on small maps, for tests
    int k3_per_cu = 2;    // persistent sort workgroups per CU
    int k1_general = 0;   // 1: always the general project+bin kernel
    int k1_stack = -1;    // fast project+bin kernel: compact survivors through the wave stack (0 / 1; -1 = by slab depth)
    int ngp_general = 0;  // 1: no in-tile NGP fold (count map + k_fold_ngp)
    int dl_quot = 1;      // maps that are not a power of two wide: allow the swept reciprocal-product quotient
    int zero_batch = 1;   // 1: the maps of a pass are cleared by one launch (0: one hipMemsetAsync each)
    int pending = 0;      // chunks per tile launch (0 = automatic: 8 ... 32 by the records a chunk brings per tile)
    int thin_host = 0;    // 1: shot-noise deviates drawn by libc rand() on the host (0: the stream continues on the device)
    int sort2 = 0;        // 1: two-level sort (project+bin sorts by coarse bin in LDS, k_sort2 by tile) where a pass
                          // qualifies.  Off by default: it moves fewer bytes but costs more instructions
    int shear_split = 0;  // 1: slicer_shear handles split every FFT into passes of <= sqrt(length) points (tests)
};
struct OptionName {
    const char *key, *env;
    int Options::*field;
};
inline const OptionName kOptionNames[] = {
    {"k4_int", "SLICER_K4_INT", &Options::k4_int},
    {"tile_log2", "SLICER_TILE_LOG2", &Options::tile_log2},
    {"tile_h_log2", "SLICER_TILE_H_LOG2", &Options::tile_h_log2},
    {"bin_batch", "SLICER_BIN_BATCH", &Options::bin_batch},
    {"unit_rows", "SLICER_UNIT_ROWS", &Options::unit_rows},
    {"k3_per_cu", "SLICER_K3_PER_CU", &Options::k3_per_cu},
    {"k1_general", "SLICER_K1_GENERAL", &Options::k1_general},
    {"k1_stack", "SLICER_K1_STACK", &Options::k1_stack},
    {"ngp_general", "SLICER_NGP_GENERAL", &Options::ngp_general},
    {"dl_quot", "SLICER_DL_QUOT", &Options::dl_quot},
    {"sort2", "SLICER_SORT2", &Options::sort2},
    {"thin_host", "SLICER_THIN_HOST", &Options::thin_host},
    {"pending", "SLICER_PENDING", &Options::pending},
    {"zero_batch", "SLICER_ZERO_BATCH", &Options::zero_batch},
    {"shear_split", "SLICER_SHEAR_SPLIT", &Options::shear_split},
};

constexpr size_t kPassScalarsBytes = sizeof(unsigned long long) * SLICER_MAX_PLANES * 6 + sizeof(int) + 7 * sizeof(unsigned);
constexpr int kBinBatch = 32768;  // particles per K1 workgroup (sweep: tools/sweep.sh)

struct slicer_handle_s {
    int device = 0;
    Options opt;
    int num_cus = 256;
    unsigned items_epoch = 0;  // launches of the tile kernel on the current w_items workspace
    hipStream_t stream = nullptr;
    bool own_stream = true;
    hipStream_t own = nullptr;
    uint64_t max_chunk = 0;
    std::string err;

    bool in_plane = false, in_file = false, finalized = false;
    slicer_plane_desc desc{};
    slicer_file_desc file{};
    uint64_t npix2 = 0;
    PlaneBufs planes[SLICER_MAX_PLANES];
    unsigned long long *d_counts = nullptr;  // [SLICER_MAX_PLANES][6]
    int *d_neg = nullptr;
    // [7] bits of the largest selected per-particle mass of this pass: per species, and slot 6 for the shared accumulator
    // (want_type_maps == 0), whose pending list mixes species -- the tile kernel's quantum must cover all of them
    unsigned *d_maxmass = nullptr;
    bool type_seen[6] = {};       // in this plane pass
    bool shared_seen = false;
    int algo_mask = 0;            // bit (1 << SLICER_ALGO_*) of every algorithm that ran in this pass; bit 3 = thinning
    bool neg_remote = false;      // another rank reported the negativity guard (slicer_reduce_meta_set)
    int file_mode[6] = {};        // NGP fold mode of the current file
    bool file_partial_flush[6] = {};  // NGP: some of this file's records of the species went to the global count map
    unsigned file_serial = 0;         // counts slicer_file_begin calls (PendingList.file_id)
    float file_mconst[6] = {};
    int fixed_exp[6] = {};
    int fixed_exp_shared = 0;
    bool fixed_exp_set[6] = {};
    bool fixed_shared_set = false;

    // host->device staging (double buffered)
    float *h_stage[2] = {nullptr, nullptr};
    float *d_stage[2] = {nullptr, nullptr};
    float *h_mstage[2] = {nullptr, nullptr};
    float *d_mstage[2] = {nullptr, nullptr};
    hipEvent_t stage_free[2] = {nullptr, nullptr};
    uint64_t stage_cap = 0;  // particles

    // SLICER_ALGO_BINNED workspace (sized for max_chunk particles)
    DevBuf w_cxy, w_cbin, w_cm, w_hist, w_hist16, w_total, w_bcount, w_items;
    DevBuf w_c1, w_sboff, w_sbstart, w_sbn;  // two-level sort: project+bin output of the current chunk
    // box sizes whose f32 quotient r/box passed (true) or failed (false) the exhaustive device sweep
    // (launch_check_box_quotient): k_project_bin_fast is only used for the former
    std::vector<std::pair<double, bool>> box_verdicts;
    std::vector<std::pair<int, bool>> dl_verdicts;  // map sizes (not powers of two) whose quot_dl3 passed / failed its sweep
    bool dl_quot_ok = false;                        // ... the verdict for the current pass's npix
    unsigned *d_sweep = nullptr;
    DevBuf w_tcounts, w_tbase, w_urand;  // shot-noise thinning (snopt > 0)
    std::vector<float> h_urand;
    // libc's rand() stream on the device (slicer_rand.hip): jump tables, the 31-word state, wave start states
    DevBuf w_randtab, w_randstate, w_randwaves;
    bool rand_tab_ready = false;
    bool rand_on_device = false;  // between thin_rng_begin and thin_rng_end the device holds the stream
    // a stream of this handle's own instead of the process-global one (slicer_rand_stream_set): the reference's MPI
    // ranks each own an identically seeded copy of libc's stream; rank threads of one process get theirs this way
    slicer::ZeroList zero_list{};      // zero-fills collected between zero_begin / zero_end
    bool zero_collect = false;
    bool rand_private = false;
    uint32_t rand_state[31] = {};
    // Process-global mode (no slicer_rand_stream_set): the process's stream is read when a pass with snopt > 0 BEGINS --
    // before that call touches the HIP runtime, whose threads draw from libc's stream themselves now and then -- the pass
    // thins from this copy, and the advanced state goes back to libc when the pass ends (flush / finalize / read, the next
    // plane_begin, destroy): whatever the runtime drew in between is overwritten.
    bool rand_pass = false;
    // snopt > 0 with several planes in one pass: the reference draws its deviates plane by plane (outer loop of
    // createDensityMaps' caller), so the chunks are kept on the device and deposited plane-major when the pass ends
    struct ThinChunk {
        int file, type;
        DevBuf pos, mass;
        uint64_t n;
    };
    struct ThinFile {
        slicer_file_desc file;
        int mode[6];
        float mconst[6];
    };
    std::vector<ThinChunk> thin_chunks;
    std::vector<ThinFile> thin_files;
    // chunks binned but not yet deposited (flushed by one k_tile_deposit launch).  One list per plane group: a pass whose
    // planes go through the binned kernels in several groups (binned_chunk) keeps every group's chunks pending separately.
    struct Pending {
        slicer::PendingList L{};
        int key = -1;        // type * 2 + has_mass (or 12 + has_mass for the shared accumulator)
        int p0 = 0, np = 0;  // planes [p0, p0 + np) of the pass are behind the pending chunks
        slicer::LaunchCfg cfg{};
        slicer::PassParams P{};
        slicer::BinGeom G{};
        slicer::Targets T{};
        uint64_t particles = 0;  // particles behind the pending chunks (bounds their record count)
        DevBuf w_sxy[slicer::kMaxPending], w_base[slicer::kMaxPending];  // one sorted slot per pending chunk
        // two-level sort: the chunk's item table (w_base then holds the items' allocation cursor), the group's bin totals
        DevBuf w_ptab[slicer::kMaxPending], w_tot;
        bool sort2 = false;
        int limit = 8;  // chunks per tile launch of this list (set when its first chunk arrives)
    };
    Pending pg[SLICER_MAX_PLANES];

    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    uint64_t prof_event_failures = 0;
    double prof_ms[KN_COUNT] = {};
    uint64_t prof_n[KN_COUNT] = {};
};

// ---- slicer_host.cpp ----
// Sets slicer_last_error of h (of the calling thread for a null h) and returns code.
int fail(slicer_handle h, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(h, e_ == hipErrorOutOfMemory ? SLICER_ERR_NOMEM : SLICER_ERR_HIP,            \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Grow-only device buffer.  *fresh (optional) is set when the buffer was (re)allocated: its contents are undefined
// (the new allocation may even reuse the old address, so callers must not compare pointers).
int ensure(slicer_handle h, DevBuf &b, size_t bytes, bool *fresh = nullptr);
void release(DevBuf &b);

// Times what is enqueued on the handle's stream during its lifetime under kernel `name` (nothing unless profiling is on).
struct ProfScope {
    slicer_handle h;
    int name;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ProfScope(slicer_handle h_, int name_);
    ~ProfScope();
};
void prof_collect(slicer_handle h);
// An event of the handle's pool (a new one while the pool is empty; null if that fails).  Whoever is done with it pushes
// it back onto h->ev_pool; slicer_destroy destroys the pool.
hipEvent_t get_event(slicer_handle h);

// What the sub-handles share.  sub_open (their *_create): the handle's stream and its device, made current; errors are
// prefixed with `who`.  sub_stream (every later call): the handle's current stream, `device` made current.
int sub_open(slicer_handle h, const char *who, hipStream_t *st, int *device);
int sub_stream(slicer_handle h, int device, hipStream_t *st);
// The device allocations of one sub-handle, freed together.
struct DevAllocs {
    std::vector<void *> ptrs;
    // rc: an earlier failure passes through and nothing is allocated, so that a *_create checks once after its last
    // call.  At least 8 bytes, so that an empty table still has an address; zero_on: cleared on that stream.
    int alloc(int rc, slicer_handle h, const char *who, void **p, size_t bytes, const hipStream_t *zero_on = nullptr);
    void replace(void *old, void *p);  // the caller freed `old` and allocated `p` in its place
    void free_all();
    ~DevAllocs() { free_all(); }
};
// What every sub-handle struct starts with (they derive from it): the parent, its device, and the device memory.
struct SubHandle {
    slicer_handle h = nullptr;
    int device = 0;
    DevAllocs mem;
};
// The npix range of a *_create whose numbers are checked before its handle: "<who>: npix must be positive", or
// "<who>: npix = <npix> above <max_npix>" (SLICER_ERR_UNSUPPORTED).
int npix_in_range(slicer_handle h, const char *who, int npix, int max_npix);
// A *_create after its argument checks: sub_open, then a T with h and device filled in (*x; null on failure).
template <class T>
int sub_new(slicer_handle h, const char *who, hipStream_t *st, T **x)
{
    *x = nullptr;
    int device = 0;
    if (int rc = sub_open(h, who, st, &device))
        return rc;
    if (!(*x = new (std::nothrow) T))
        return fail(h, SLICER_ERR_NOMEM, "out of host memory");
    (*x)->h = h;
    (*x)->device = device;
    return SLICER_OK;
}
// ... and its end: rc of the allocations and uploads; x goes to the caller, or is deleted.
template <class T>
int sub_done(int rc, T *x, T **out)
{
    if (rc != SLICER_OK) {
        delete x;
        return rc;
    }
    *out = x;
    return SLICER_OK;
}
// `bytes` from `dev` to `host` on the parent's stream, and wait for them: what a *_read, *_read_map or *_spectrum ends in.
int sub_read(const SubHandle &s, void *host, const void *dev, size_t bytes);
// A *_destroy: waits for the parent's stream, then deletes.  Null: SLICER_ERR_ARG and no error text.
template <class T>
int sub_destroy(T *x)
{
    if (!x)
        return SLICER_ERR_ARG;
    (void)hipSetDevice(x->device);
    (void)hipStreamSynchronize(x->h->stream);
    delete x;
    return SLICER_OK;
}
inline bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes)
{
    return (uintptr_t)a < (uintptr_t)b + b_bytes && (uintptr_t)b < (uintptr_t)a + a_bytes;
}
bool fft_size_supported(int n);  // 2 <= n <= kFftMaxN (slicer_fft.hpp) with prime factors 2, 3, 5, 7 only: what slicer_fft_create plans

// ---- pass_plan.cpp ----
inline bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }
int acc_kind(const slicer_plane_desc &d, bool has_mass);
slicer::LaunchCfg launch_cfg(const slicer_plane_desc &d, bool has_mass);
void make_params(slicer_handle h, int type, bool has_mass, slicer::PassParams &P);
int pick_fixed_exp(const slicer_plane_desc &d, double m, bool has_mass);
void fill_targets(slicer_handle h, int type, bool has_mass, slicer::Targets &T);
// Planes [p0, p0 + np) of (P, T) move to slots 0 .. np - 1.  narrow: the pass shrinks to them (n_planes = np and the
// slots beyond select nothing, as make_params leaves unused slots); otherwise every other field stays as it is.
void planes_to_front(slicer::PassParams &P, slicer::Targets &T, int p0, int np, bool narrow);
int rep_windows(int nrmax);
int rep_window_side(int nrmax);
bool choose_geom(const slicer_plane_desc &d, int acc, const Options &opt, slicer::BinGeom &G);
int dl_quotient_ok(slicer_handle h, int npix, bool &ok, unsigned *examples9 = nullptr);
int k1_fast_args(slicer_handle h, const slicer::PassParams &P, const slicer::BinGeom &G, int nblocks, slicer::K1Args &A,
                 bool &fast);

// ---- binned_pass.cpp ----
int zero_async(slicer_handle h, void *p, size_t bytes);
void zero_begin(slicer_handle h);
int zero_end(slicer_handle h);
int prepare_type(slicer_handle h, int type, bool has_mass);
bool ngp_foldable(slicer_handle h, int type);
void ngp_spoil_file(slicer_handle h, int type);
int flush_pending(slicer_handle h);
int deposit_device_chunk(slicer_handle h, int type, const float *d_pos, const float *d_mass, uint64_t n);
int fold_file_plane(slicer_handle h, int p);

// ---- thinning.cpp ----
void pass_stream_return(slicer_handle h);
bool thin_deferred(slicer_handle h);
void thin_drop(slicer_handle h);
int thin_replay(slicer_handle h);
// one chunk of a pass with snopt > 0: deposited now (one plane) or kept for thin_replay (several)
int thin_deposit_chunk(slicer_handle h, int type, const slicer::PassParams &P, const slicer::Targets &T,
                       const slicer::LaunchCfg &cfg, const float *d_pos, const float *d_mass, uint64_t n);

// ---- slicer_capi.cpp ----
int check_deposit_args(slicer_handle h, int type, const void *pos, const void *mass, uint64_t n);

#pragma GCC visibility pop
