// thinning.cpp -- shot-noise thinning (snopt > 0, densitymaps.cpp:387-397) and libc's rand() stream behind it: on the
// host, continued on the device, private to a handle or the process's own.
#include "slicer_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

using namespace slicer;

// End of a pass in process-global mode: libc gets its stream back, advanced by the pass's draws.
void pass_stream_return(slicer_handle h)
{
    if (h->rand_pass) {
        (void)libc_rand_put(h->rand_state);
        h->rand_pass = false;
    }
}

namespace {

// The libc stream moves to the device for a run of thinned chunks: thin_rng_begin reads the process-global generator
// state and uploads it, thin_rng_end brings the advanced state back and installs it (one synchronisation).  False from
// begin: the stream stays on the host (option thin_host, a generator other than glibc's TYPE_3, or the layout check of
// slicer_rand.hip failed) and thin_chunk draws with rand() as the reference does.
bool thin_rng_begin(slicer_handle h, int &rc)
{
    rc = SLICER_OK;
    if (h->opt.thin_host)
        return false;
    uint32_t v[31];
    if (h->rand_private || h->rand_pass)
        memcpy(v, h->rand_state, sizeof v);
    else if (!libc_rand_grab(v))
        return false;
    if ((rc = ensure(h, h->w_randtab, rand_tables_bytes())) || (rc = ensure(h, h->w_randstate, 32 * 4)))
        return false;
    if (!h->rand_tab_ready) {
        if (rand_tables_upload(h->w_randtab.p, h->stream) != hipSuccess) {
            rc = fail(h, SLICER_ERR_HIP, "upload of the generator tables failed: %s", hipGetErrorString(hipGetLastError()));
            return false;
        }
        h->rand_tab_ready = true;
    }
    if (hipMemcpyAsync(h->w_randstate.p, v, sizeof v, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {  // v is a stack array
        rc = fail(h, SLICER_ERR_HIP, "upload of the generator state failed: %s", hipGetErrorString(hipGetLastError()));
        return false;
    }
    h->rand_on_device = true;
    return true;
}

int thin_rng_end(slicer_handle h)
{
    if (!h->rand_on_device)
        return SLICER_OK;
    h->rand_on_device = false;
    uint32_t v[31];
    HIPCHK(h, hipMemcpyAsync(v, h->w_randstate.p, sizeof v, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->rand_private || h->rand_pass)
        memcpy(h->rand_state, v, sizeof v);
    else if (!libc_rand_put(v))
        return fail(h, SLICER_ERR_STATE, "the process changed its libc generator during a thinned pass");
    return SLICER_OK;
}

// Shot-noise thinning of one chunk into plane slot 0 of (P, T).
int thin_chunk(slicer_handle h, PassParams P, const Targets &T, const LaunchCfg &cfg, const float *d_pos,
               const float *d_mass, uint64_t n)
{
    // densitymaps.cpp:387-397: one libc rand() per selected entry, in selection order.  Count on the device, then
    // either continue the process-global stream on the device (thin_rng_begin) or draw on the host from it -- the
    // same deviates either way, exactly what the reference consumes -- and deposit.
    P.series_max = kSeriesMax15;  // no pre-test on this path either
    const uint64_t nchunks = (n + 63) / 64;
    int rc;
    if ((rc = ensure(h, h->w_tcounts, nchunks * 4)) || (rc = ensure(h, h->w_tbase, (nchunks + 1) * 8)))
        return rc;
    {
        ProfScope ps(h, KN_DIRECT);
        HIPCHK(h, launch_thin_count(d_pos, n, P, (unsigned *)h->w_tcounts.p, (unsigned long long *)h->w_tbase.p,
                                    h->d_neg, h->stream));
    }
    const double pw = std::pow(2, h->desc.snopt);
    const unsigned long long *d_nsel = (unsigned long long *)h->w_tbase.p + nchunks;
    const uint64_t reps = (uint64_t)(2 * P.nrep[0] + 1) * (uint64_t)(2 * P.nrep[0] + 1);
    const bool on_device = h->rand_on_device;
    // at most one draw per (particle, replica); with lateral replicas the buffer is sized by the real count
    unsigned long long max_draws = n * reps;
    if (on_device) {
        if (reps > 1) {
            HIPCHK(h, hipMemcpyAsync(&max_draws, d_nsel, sizeof max_draws, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        if ((rc = ensure(h, h->w_urand, std::max<size_t>(max_draws, 1) * 4)) ||
            (rc = ensure(h, h->w_randwaves, rand_wave_states_bytes(max_draws))))
            return rc;
    } else {
        unsigned long long nsel = 0;
        HIPCHK(h, hipMemcpyAsync(&nsel, d_nsel, sizeof nsel, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->h_urand.resize(nsel);
        if (h->rand_private || h->rand_pass)
            libc_rand_model_fill(h->rand_state, h->h_urand.data(), nsel);
        else
            for (unsigned long long k = 0; k < nsel; k++)
                h->h_urand[k] = rand() / float(RAND_MAX);
        if ((rc = ensure(h, h->w_urand, std::max<size_t>(nsel, 1) * 4)))
            return rc;
        if (nsel)
            HIPCHK(h, hipMemcpyAsync(h->w_urand.p, h->h_urand.data(), nsel * 4, hipMemcpyHostToDevice, h->stream));
    }
    {
        ProfScope ps(h, KN_DIRECT);  // (with the generator, where it runs on the device)
        if (on_device)
            HIPCHK(h, launch_rand_deviates(d_nsel, (uint32_t *)h->w_randstate.p, (uint32_t *)h->w_randwaves.p,
                                           h->w_randtab.p, (float *)h->w_urand.p, max_draws, h->stream));
        HIPCHK(h, launch_thin_deposit(cfg, d_pos, d_mass, n, P, T, (const unsigned long long *)h->w_tbase.p,
                                      (const float *)h->w_urand.p, 1. / pw, pw, h->stream));
    }
    if (!on_device)
        HIPCHK(h, hipStreamSynchronize(h->stream));  // h_urand is reused by the next chunk
    h->algo_mask |= on_device ? (1 << 3) | (1 << 8) : 1 << 3;
    return SLICER_OK;
}

}  // namespace

bool thin_deferred(slicer_handle h) { return h->desc.snopt > 0 && h->desc.n_planes > 1; }

void thin_drop(slicer_handle h)
{
    for (auto &c : h->thin_chunks) {
        release(c.pos);
        release(c.mass);
    }
    h->thin_chunks.clear();
    h->thin_files.clear();
}

// snopt > 0 with several planes: deposit the retained chunks plane-major, files and species in their original order
// inside each plane -- the order in which the reference (one createDensityMaps call per plane) consumes rand().
static int thin_replay_chunks(slicer_handle h);

// Called wherever a pass ends (flush / finalize / read): deposits the retained chunks of a multi-plane thinned pass and
// hands libc its stream back.
int thin_replay(slicer_handle h)
{
    const int rc = thin_replay_chunks(h);
    pass_stream_return(h);
    return rc;
}

static int thin_replay_chunks(slicer_handle h)
{
    if (!thin_deferred(h) || (h->thin_chunks.empty() && h->thin_files.empty()))
        return SLICER_OK;
    const slicer_plane_desc &d = h->desc;
    const slicer_file_desc file_saved = h->file;
    int rc = SLICER_OK;
    thin_rng_begin(h, rc);  // (false: the deviates come from the host loop)
    for (int p = 0; p < d.n_planes && !rc; p++) {
        size_t ci = 0;
        for (size_t f = 0; f < h->thin_files.size() && !rc; f++) {
            const auto &F = h->thin_files[f];
            h->file = F.file;
            for (int t = 0; t < 6; t++) {
                h->file_mode[t] = F.mode[t];
                h->file_mconst[t] = F.mconst[t];
            }
            for (; ci < h->thin_chunks.size() && h->thin_chunks[ci].file == (int)f && !rc; ci++) {
                const auto &c = h->thin_chunks[ci];
                const bool has_mass = c.mass.p != nullptr;
                PassParams P;
                make_params(h, c.type, has_mass, P);
                Targets T;
                fill_targets(h, c.type, has_mass, T);
                planes_to_front(P, T, p, 1, false);  // thin_chunk works on slot 0
                rc = thin_chunk(h, P, T, launch_cfg(d, has_mass), (const float *)c.pos.p, (const float *)c.mass.p, c.n);
            }
            if (!rc && d.mas == SLICER_MAS_NGP)
                rc = fold_file_plane(h, p);
        }
    }
    const int rce = thin_rng_end(h);
    rc = rc ? rc : rce;
    h->file = file_saved;
    for (int t = 0; t < 6; t++)
        h->file_mode[t] = 0;
    thin_drop(h);
    return rc;
}

int thin_deposit_chunk(slicer_handle h, int type, const PassParams &P, const Targets &T, const LaunchCfg &cfg,
                       const float *d_pos, const float *d_mass, uint64_t n)
{
    const slicer_plane_desc &d = h->desc;
    const bool has_mass = d_mass != nullptr;
    if (d.n_planes == 1) {
        if (d.mas == SLICER_MAS_NGP)
            ngp_spoil_file(h, type);  // counts into the global map: the file's fold is k_fold_ngp's, not the tile kernel's
        int rc = SLICER_OK;
        thin_rng_begin(h, rc);
        if (!rc)
            rc = thin_chunk(h, P, T, cfg, d_pos, d_mass, n);
        const int rce = thin_rng_end(h);  // the host's stream is current again before the call returns
        return rc ? rc : rce;
    }
    // several planes: keep the chunk, thin_replay deposits it once per plane in the reference's order
    slicer_handle_s::ThinChunk c{};
    c.file = (int)h->thin_files.size();
    c.type = type;
    c.n = n;
    int rc = ensure(h, c.pos, n * 12);
    if (!rc && has_mass)
        rc = ensure(h, c.mass, n * 4);
    if (rc) {
        release(c.pos);
        release(c.mass);
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(c.pos.p, d_pos, n * 12, hipMemcpyDeviceToDevice, h->stream));
    if (has_mass)
        HIPCHK(h, hipMemcpyAsync(c.mass.p, d_mass, n * 4, hipMemcpyDeviceToDevice, h->stream));
    h->thin_chunks.push_back(c);
    return SLICER_OK;
}

extern "C" {

int slicer_rand_stream_set(slicer_handle h, const uint32_t *v31)
{
    if (!h)
        return fail(h, SLICER_ERR_ARG, "null handle");
    if (h->in_file)
        return fail(h, SLICER_ERR_STATE, "slicer_rand_stream_set inside a file");
    pass_stream_return(h);
    h->rand_private = v31 != nullptr;
    if (v31)
        memcpy(h->rand_state, v31, sizeof h->rand_state);
    return SLICER_OK;
}

int slicer_rand_stream_get(slicer_handle h, uint32_t *v31)
{
    if (!h || !v31)
        return fail(h, SLICER_ERR_ARG, "null argument");
    if (!h->rand_private)
        return fail(h, SLICER_ERR_STATE, "the handle draws from the process-global stream (slicer_rand_stream_set)");
    memcpy(v31, h->rand_state, sizeof h->rand_state);
    return SLICER_OK;
}

int slicer_libc_rand_supported(void)
{
    uint32_t v[31];
    return libc_rand_grab(v) ? 1 : 0;
}

int slicer_libc_rand_state_get(uint32_t *v31)
{
    if (!v31)
        return fail(nullptr, SLICER_ERR_ARG, "null argument");
    return libc_rand_grab(v31) ? SLICER_OK : fail(nullptr, SLICER_ERR_UNSUPPORTED, "libc generator state not accessible");
}

int slicer_libc_rand_state_set(const uint32_t *v31)
{
    if (!v31)
        return fail(nullptr, SLICER_ERR_ARG, "null argument");
    return libc_rand_put(v31) ? SLICER_OK : fail(nullptr, SLICER_ERR_UNSUPPORTED, "libc generator state not accessible");
}

}  // extern "C"
