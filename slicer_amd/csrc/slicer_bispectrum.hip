// slicer_bispectrum.hip -- on-device binned bispectra of a kappa map.
//
// With khat = rfft2(kappa) in f64 (slicer_fft.hip, the transform shared with the shear handle) and the bins of slicer_power_bins
// minus the mode m2 = 0: F_b = irfft2(khat 1[mode in b]) and I_b = irfft2(1[mode in b]), both kept in f64
// (slicer_fft_inverse_band), and for a triple i <= j <= k
//   S_ijk = sum_x F_i F_j F_k,   T_ijk = n^4 sum_x I_i I_j I_k,   B_ijk = theta^4 / n^6 * (n^4 S_ijk) / T_ijk.
// T depends only on the geometry: it is contracted once, at create, through the buffer that later holds the F_b.
// The results must not depend on the shear_split option, which reorders the transform's butterflies and with them its
// last bits: everything is computed with the unsplit plan, and with shear_split = 1 a second, split plan transforms the
// map once more, only for the spectrum that slicer_bispectrum_spectrum reports (bitwise the shear handle's under the
// same setting).
//
// The contraction is a tall-skinny product: rows (i, j), columns k, depth n^2.  k_bispectrum: lanes are pixels, and a
// wave owns one item -- a register tile of one i, up to kRJ of its j and up to kKB of their k -- over one chunk of
// pixels.  Per pixel it loads F_i, the F_j and the F_k once (wave-wide contiguous reads off uniform bases: 1 + kRJ + kKB
// loads for kRJ kKB products), forms P_r = F_i F_j[r] and adds P_r F_k[c] to the accumulator of slot (r, c); the
// accumulators and the F values stay in registers under static indexing.  The kernel is bound by these loads, which
// come from L2 (every item streams its maps again), so the tile is as large as the registers take (DESIGN.md, N15 cost).
// A lane sums blocks of kInner products in registers and adds every block to a second accumulator, its own cell of
// LDS, so no running sum is longer than kInner terms plus the blocks of one chunk; one xor butterfly per slot ends the
// chunk, and lane 0 stores the partial at [chunk][unique triple].  The waves of a workgroup take adjacent items of the
// same chunk, which mostly share i.
// k_bispectrum_finish: one wave per list entry, lane l adds a contiguous run of its triple's chunks in index order, then
// the same butterfly.  No atomics; the order of every triple's sum is fixed by npix alone, so it is bitwise repeatable
// and does not depend on which other triples are in the list (a slot never reads another slot's accumulator).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_power_internal.hpp"
#include "slicer_host.hpp"

namespace {

constexpr int kMaxBins = SLICER_BISPECTRUM_MAX_BINS;
constexpr int kMaxTriples = 1 << 20;
constexpr int kMaxNpixHost = 16384;  // slicer_bispectrum_triangles: the full-plane table has npix^2 bytes
constexpr int kRJ = 4, kKB = 8;      // the register tile of one wave: j rows x k columns
constexpr int kThreads = 128;
constexpr int kWaves = kThreads / 64;
constexpr int kInner = 64;       // products of a lane's inner block
constexpr int kMinChunk = 4096;  // pixels per chunk, at least; at most kMaxChunks chunks
constexpr int kMaxChunks = 1024;
constexpr int64_t kWorkLimit = (int64_t)1 << 31;

struct Item {
    int i;
    int j[kRJ];          // unused rows repeat j[0]
    int k[kKB];          // unused columns repeat k[0]
    int slot[kRJ][kKB];  // the unique triple (i, j[r], k[c]); -1: not in the list
};

struct ContractArgs {
    const double *F;  // [B][npix2]
    const Item *items;
    double *partial;  // [nchunks][nuniq]
    size_t npix2;
    int nitems, nuniq, chunk;  // chunk: pixels per blockIdx.y, a multiple of 64
};

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off /= 2)
        v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void k_bispectrum(ContractArgs a)
{
    __shared__ double outer[kRJ * kKB][kThreads];  // every thread's own second-level accumulators
    const int tid = threadIdx.x, lane = tid % 64, it = blockIdx.x * kWaves + tid / 64;
    if (it >= a.nitems)
        return;
    const Item &item = a.items[it];
    const double *Fi = a.F + (size_t)item.i * a.npix2;
    const double *Fj[kRJ], *Fk[kKB];
#pragma unroll
    for (int r = 0; r < kRJ; r++)
        Fj[r] = a.F + (size_t)item.j[r] * a.npix2;
#pragma unroll
    for (int c = 0; c < kKB; c++)
        Fk[c] = a.F + (size_t)item.k[c] * a.npix2;
    const size_t x0 = (size_t)blockIdx.y * a.chunk + lane;
    const int steps = a.chunk / 64;
    for (int b0 = 0; b0 < steps; b0 += kInner) {
        const int b1 = min(b0 + kInner, steps);
        double acc[kRJ][kKB];
#pragma unroll
        for (int r = 0; r < kRJ; r++)
#pragma unroll
            for (int c = 0; c < kKB; c++)
                acc[r][c] = 0.0;
        for (int b = b0; b < b1; b++) {
            const size_t x = x0 + (size_t)b * 64;
            const bool in = x < a.npix2;
            const double fi = in ? Fi[x] : 0.0;
            double p[kRJ], f[kKB];
#pragma unroll
            for (int r = 0; r < kRJ; r++)
                p[r] = fi * (in ? Fj[r][x] : 0.0);
#pragma unroll
            for (int c = 0; c < kKB; c++)
                f[c] = in ? Fk[c][x] : 0.0;
#pragma unroll
            for (int r = 0; r < kRJ; r++)
#pragma unroll
                for (int c = 0; c < kKB; c++)
                    acc[r][c] += p[r] * f[c];
        }
#pragma unroll
        for (int r = 0; r < kRJ; r++)
#pragma unroll
            for (int c = 0; c < kKB; c++)
                outer[r * kKB + c][tid] = b0 == 0 ? acc[r][c] : outer[r * kKB + c][tid] + acc[r][c];
    }
#pragma unroll
    for (int r = 0; r < kRJ; r++)
#pragma unroll
        for (int c = 0; c < kKB; c++) {
            const double v = wave_sum(outer[r * kKB + c][tid]);
            if (lane == 0 && item.slot[r][c] >= 0)
                a.partial[(size_t)blockIdx.y * a.nuniq + item.slot[r][c]] = v;
        }
}

// sums[t] = the partials of list entry t's unique triple over the chunks: lane l adds chunks l per ... (l + 1) per - 1
// in order
__global__ __launch_bounds__(kThreads) void k_bispectrum_finish(const double *partial, const int *uniq_of, int nchunks,
                                                                int nuniq, int nslots, double *sums)
{
    const int lane = threadIdx.x % 64, t = blockIdx.x * kWaves + threadIdx.x / 64;
    if (t >= nslots)
        return;
    const int u = uniq_of[t];
    const int per = (nchunks + 63) / 64, c0 = min(lane * per, nchunks), c1 = min(c0 + per, nchunks);
    double v = 0.0;
    for (int c = c0; c < c1; c++)
        v += partial[(size_t)c * nuniq + u];
    v = wave_sum(v);
    if (lane == 0)
        sums[t] = v;
}

struct Triple {
    int i, j, k;
};

// The list, or all B (B + 1) (B + 2) / 6 triples in lexicographic order for NULL (then n must be that number); "" if
// it is usable, else why not.
const char *check_triples(int B, int64_t n, const int32_t *triples, std::vector<Triple> &out)
{
    out.clear();
    if (!triples) {
        if (n != (int64_t)B * (B + 1) * (B + 2) / 6)
            return "n_triples must be B (B + 1) (B + 2) / 6 for all triples (triples = NULL)";
        for (int i = 0; i < B; i++)
            for (int j = i; j < B; j++)
                for (int k = j; k < B; k++)
                    out.push_back({i, j, k});
        return "";
    }
    if (n < 1)
        return "fewer than 1 triple";
    for (int64_t t = 0; t < n; t++) {
        const int i = triples[3 * t], j = triples[3 * t + 1], k = triples[3 * t + 2];
        if (!(0 <= i && i <= j && j <= k && k < B))
            return "a triple is not 0 <= i <= j <= k < the number of bins";
        out.push_back({i, j, k});
    }
    return "";
}

// The distinct triples of the list in ascending order, and for every list entry its index among them.
std::vector<Triple> unique_triples(const std::vector<Triple> &tr, std::vector<int> &uniq_of)
{
    auto less = [](const Triple &x, const Triple &y) { return x.i != y.i ? x.i < y.i : x.j != y.j ? x.j < y.j : x.k < y.k; };
    std::vector<Triple> u(tr);
    std::sort(u.begin(), u.end(), less);
    u.erase(std::unique(u.begin(), u.end(), [&](const Triple &x, const Triple &y) { return !less(x, y) && !less(y, x); }),
            u.end());
    uniq_of.resize(tr.size());
    for (size_t t = 0; t < tr.size(); t++)
        uniq_of[t] = (int)(std::lower_bound(u.begin(), u.end(), tr[t], less) - u.begin());
    return u;
}

// The register tiles of the distinct, sorted triples: per i the distinct j in groups of kRJ, per group the k that any of
// its j needs in blocks of kKB.
std::vector<Item> make_items(const std::vector<Triple> &u)
{
    std::vector<Item> items;
    for (size_t a = 0; a < u.size();) {
        size_t e = a;  // [a, e): the triples of one i
        while (e < u.size() && u[e].i == u[a].i)
            e++;
        std::vector<int> js;
        for (size_t t = a; t < e; t++)
            if (js.empty() || js.back() != u[t].j)
                js.push_back(u[t].j);
        for (size_t g = 0; g < js.size(); g += kRJ) {
            const size_t g1 = std::min(js.size(), g + kRJ);
            std::vector<int> ks;
            for (size_t t = a; t < e; t++)
                if (u[t].j >= js[g] && u[t].j <= js[g1 - 1])
                    ks.push_back(u[t].k);
            std::sort(ks.begin(), ks.end());
            ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
            for (size_t q = 0; q < ks.size(); q += kKB) {
                const size_t q1 = std::min(ks.size(), q + kKB);
                Item it{};
                it.i = u[a].i;
                for (int r = 0; r < kRJ; r++)
                    it.j[r] = js[std::min(g + r, g1 - 1)];
                for (int c = 0; c < kKB; c++)
                    it.k[c] = ks[std::min(q + c, q1 - 1)];
                bool any = false;
                for (int r = 0; r < kRJ; r++)
                    for (int c = 0; c < kKB; c++) {
                        it.slot[r][c] = -1;
                        if (g + r >= g1 || q + c >= q1)
                            continue;
                        const Triple want{it.i, it.j[r], it.k[c]};
                        for (size_t t = a; t < e; t++)
                            if (u[t].j == want.j && u[t].k == want.k) {
                                it.slot[r][c] = (int)t;
                                any = true;
                            }
                    }
                if (any)
                    items.push_back(it);
            }
        }
        a = e;
    }
    return items;
}

}  // namespace

struct slicer_bispectrum_s : SubHandle {
    slicer_fft_s *fft = nullptr;        // the unsplit plan: every result comes from it
    slicer_fft_s *fft_split = nullptr;  // shear_split = 1 only: the plan of spec_split
    int n = 0, H = 0, B = 0, nslots = 0, nuniq = 0, nitems = 0, nchunks = 0, chunk = 0;
    double norm = 0.0;  // theta^4 / n^6
    std::vector<double> e2;  // edge squares, B + 1
    std::vector<double> T;   // [nslots]
    double2 *spec = nullptr;
    double2 *spec_split = nullptr;  // shear_split = 1 only: what slicer_bispectrum_spectrum reports
    double *F = nullptr;  // [B][n^2]: the I_b during create, then the F_b of the last run
    Item *items = nullptr;
    int *uniq_of = nullptr;  // [nslots]: the unique triple of every list entry
    double *partial = nullptr, *sums = nullptr;
    bool ran = false;
    SLICER_FFT_INTERNAL ~slicer_bispectrum_s()
    {
        slicer_fft_destroy(fft);
        slicer_fft_destroy(fft_split);
    }
};

namespace {

// the B band inverses of `spec` (NULL: of the bands themselves) into bh->F, then the sums of every slot into bh->sums
int contract(slicer_bispectrum_handle bh, hipStream_t st, const double2 *spec)
{
    const size_t npix2 = (size_t)bh->n * bh->n;
    {
        ProfScope ps(bh->h, KN_BISPECTRUM_BAND);
        for (int b = 0; b < bh->B; b++)
            if (int rc = slicer_fft_inverse_band(bh->fft, st, spec, bh->e2[b], bh->e2[b + 1], b == bh->B - 1,
                                                 bh->F + (size_t)b * npix2))
                return rc;
    }
    {
        ProfScope ps(bh->h, KN_BISPECTRUM);
        ContractArgs a{};
        a.F = bh->F;
        a.items = bh->items;
        a.partial = bh->partial;
        a.npix2 = npix2;
        a.nitems = bh->nitems;
        a.nuniq = bh->nuniq;
        a.chunk = bh->chunk;
        const dim3 grid((unsigned)((bh->nitems + kWaves - 1) / kWaves), (unsigned)bh->nchunks);
        hipLaunchKernelGGL(k_bispectrum, grid, dim3(kThreads), 0, st, a);
        HIPCHK(bh->h, hipGetLastError());
    }
    {
        ProfScope ps(bh->h, KN_BISPECTRUM_FINISH);
        hipLaunchKernelGGL(k_bispectrum_finish, dim3((unsigned)((bh->nslots + kWaves - 1) / kWaves)), dim3(kThreads), 0, st,
                           bh->partial, bh->uniq_of, bh->nchunks, bh->nuniq, bh->nslots, bh->sums);
        HIPCHK(bh->h, hipGetLastError());
    }
    return SLICER_OK;
}

}  // namespace

int slicer_bispectrum_triangles(int32_t npix, int32_t n_edges, const double *edges, int32_t n_triples,
                                const int32_t *triples, int64_t *out)
{
    const char *who = "slicer_bispectrum_triangles";
    if (npix < 1 || npix > kMaxNpixHost || !out)
        return fail(nullptr, SLICER_ERR_ARG, "%s: npix out of 1..%d, or null output", who, kMaxNpixHost);
    std::vector<double> e;
    const char *why = check_edges(npix, n_edges, edges, e);
    if (*why)
        return fail(nullptr, SLICER_ERR_ARG, "%s: %s", who, why);
    const int n = npix, B = n_edges - 1;
    std::vector<Triple> tr;
    why = check_triples(B, n_triples, triples, tr);
    if (*why)
        return fail(nullptr, SLICER_ERR_ARG, "%s: %s", who, why);
    // the bin of every mode of the full plane (-1: none), and the modes of every bin
    std::vector<double> e2(B + 1);
    for (int b = 0; b <= B; b++)
        e2[b] = e[b] * e[b];
    std::vector<int16_t> bin((size_t)n * n, -1);
    std::vector<std::vector<int32_t>> modes(B);  // i0 * n + i1
    for (int i0 = 0; i0 < n; i0++) {
        const double s0 = (double)(i0 < (n + 1) / 2 ? i0 : i0 - n);
        for (int i1 = 0; i1 < n; i1++) {
            const double s1 = (double)(i1 < (n + 1) / 2 ? i1 : i1 - n), m2 = s0 * s0 + s1 * s1;
            if (m2 == 0.0)
                continue;
            int b = (int)(std::upper_bound(e2.begin(), e2.end(), m2) - e2.begin()) - 1;  // last edge <= m2
            if (b == B && m2 == e2[B])
                b = B - 1;
            if (b < 0 || b >= B)
                continue;
            bin[(size_t)i0 * n + i1] = (int16_t)b;
            modes[b].push_back(i0 * n + i1);
        }
    }
    int64_t work = 0;
    for (const Triple &t : tr) {
        work += (int64_t)modes[t.i].size() * (int64_t)modes[t.j].size();
        if (work > kWorkLimit)
            return fail(nullptr, SLICER_ERR_UNSUPPORTED,
                        "%s: more than 2^31 mode pairs to enumerate (the sum of N_i N_j over the triples)", who);
    }
    // per (i, j) prefix of the list: the bins of -l1 - l2 over every l1 in i and l2 in j
    std::vector<int> order(tr.size());
    for (size_t t = 0; t < tr.size(); t++)
        order[t] = (int)t;
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return tr[a].i != tr[b].i ? tr[a].i < tr[b].i : tr[a].j < tr[b].j; });
    std::vector<int64_t> hist(B);
    int pi = -1, pj = -1;
    for (int t : order) {
        if (tr[t].i != pi || tr[t].j != pj) {
            pi = tr[t].i;
            pj = tr[t].j;
            std::fill(hist.begin(), hist.end(), 0);
            for (int32_t l1 : modes[pi]) {
                const int a0 = l1 / n, a1 = l1 % n;
                for (int32_t l2 : modes[pj]) {
                    const int c0 = (2 * n - a0 - l2 / n) % n, c1 = (2 * n - a1 - l2 % n) % n;
                    const int b = bin[(size_t)c0 * n + c1];
                    if (b >= 0)
                        hist[b]++;
                }
            }
        }
        out[t] = hist[tr[t].k];
    }
    return SLICER_OK;
}

int slicer_bispectrum_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_edges, const double *edges,
                             int32_t n_triples, const int32_t *triples, slicer_bispectrum_handle *out)
{
    const char *who = "slicer_bispectrum_create";
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (!fft_size_supported(npix))
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: npix = %d unsupported (2..16384, prime factors 2, 3, 5, 7 only)", who,
                    npix);
    if (n_edges - 1 > kMaxBins)
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: %d bins, at most %d", who, n_edges - 1, kMaxBins);
    std::vector<double> e;
    const char *why = check_edges(npix, n_edges, edges, e);
    if (*why)
        return fail(h, SLICER_ERR_ARG, "%s: %s", who, why);
    const int n = npix, H = n / 2 + 1, B = n_edges - 1;
    std::vector<Triple> tr;
    why = check_triples(B, n_triples, triples, tr);
    if (*why)
        return fail(h, SLICER_ERR_ARG, "%s: %s", who, why);
    if (tr.size() > (size_t)kMaxTriples)
        return fail(h, SLICER_ERR_UNSUPPORTED, "%s: %zu triples, at most %d", who, tr.size(), kMaxTriples);
    if (!std::isfinite(angle_deg) || angle_deg <= 0.0)
        return fail(h, SLICER_ERR_ARG, "%s: the angle must be positive and finite", who);
    hipStream_t st = nullptr;
    slicer_bispectrum_handle bh = nullptr;
    if (int rc = sub_new(h, who, &st, &bh))
        return rc;
    bh->n = n;
    bh->H = H;
    bh->B = B;
    bh->nslots = (int)tr.size();
    const double theta = angle_deg * M_PI / 180.0, dn = (double)n;
    bh->norm = theta * theta * theta * theta / (dn * dn * dn * dn * dn * dn);
    bh->e2.resize(B + 1);
    for (int b = 0; b <= B; b++)
        bh->e2[b] = e[b] * e[b];
    std::vector<int> uniq_of;
    const std::vector<Triple> uniq = unique_triples(tr, uniq_of);
    const std::vector<Item> items = make_items(uniq);
    bh->nuniq = (int)uniq.size();
    bh->nitems = (int)items.size();
    const size_t npix2 = (size_t)n * n;
    const size_t want = std::min<size_t>(kMaxChunks, (npix2 + kMinChunk - 1) / kMinChunk);
    bh->chunk = (int)(((npix2 + want - 1) / want + 63) / 64 * 64);
    bh->nchunks = (int)((npix2 + bh->chunk - 1) / bh->chunk);

    int rc = slicer_fft_create(h, n, 0, st, bh->device, who, &bh->fft);
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->spec, (size_t)n * H * sizeof(double2));
    if (h->opt.shear_split) {
        if (rc == SLICER_OK)
            rc = slicer_fft_create(h, n, 1, st, bh->device, who, &bh->fft_split);
        rc = bh->mem.alloc(rc, h, who, (void **)&bh->spec_split, (size_t)n * H * sizeof(double2));
    }
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->F, (size_t)B * npix2 * sizeof(double));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->items, items.size() * sizeof(Item));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->uniq_of, uniq_of.size() * sizeof(int));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->partial, (size_t)bh->nchunks * bh->nuniq * sizeof(double));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->sums, (size_t)bh->nslots * sizeof(double));
    if (rc == SLICER_OK) {
        hipError_t err = hipMemcpyAsync(bh->items, items.data(), items.size() * sizeof(Item), hipMemcpyHostToDevice, st);
        if (err == hipSuccess)
            err = hipMemcpyAsync(bh->uniq_of, uniq_of.data(), uniq_of.size() * sizeof(int), hipMemcpyHostToDevice, st);
        if (err != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: upload: %s", who, hipGetErrorString(err));
    }
    // T: the contraction of the I_b, which the first run overwrites with its F_b
    if (rc == SLICER_OK)
        rc = contract(bh, st, nullptr);
    if (rc == SLICER_OK) {
        bh->T.resize(bh->nslots);
        hipError_t err = hipMemcpyAsync(bh->T.data(), bh->sums, bh->T.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        if (err == hipSuccess)
            err = hipStreamSynchronize(st);  // also: `items` and `uniq_of` are host temporaries
        if (err != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: the triangle counts: %s", who, hipGetErrorString(err));
        const double n4 = dn * dn * dn * dn;
        for (double &t : bh->T)
            t = n4 * t;
    }
    if (rc != SLICER_OK)
        (void)hipStreamSynchronize(st);
    return sub_done(rc, bh, out);
}

int slicer_bispectrum_run(slicer_bispectrum_handle bh, const float *d_map)
{
    if (!bh || !d_map)
        return fail(bh ? bh->h : nullptr, SLICER_ERR_ARG, "slicer_bispectrum_run: null argument");
    hipStream_t st;
    if (int rc = sub_stream(bh->h, bh->device, &st))
        return rc;
    bh->ran = false;
    {
        ProfScope ps(bh->h, KN_BISPECTRUM_FFT);
        if (int rc = slicer_fft_forward(bh->fft, st, d_map, bh->spec))
            return rc;
        if (bh->fft_split)
            if (int rc = slicer_fft_forward(bh->fft_split, st, d_map, bh->spec_split))
                return rc;
    }
    if (int rc = contract(bh, st, bh->spec))
        return rc;
    bh->ran = true;
    return SLICER_OK;
}

int slicer_bispectrum_read(slicer_bispectrum_handle bh, double *b, double *triangles, double *sums)
{
    if (!bh)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_bispectrum_read: null handle");
    if ((b || sums) && !bh->ran)
        return fail(bh->h, SLICER_ERR_STATE, "slicer_bispectrum_read of b or sums before any slicer_bispectrum_run");
    hipStream_t st;
    if (int rc = sub_stream(bh->h, bh->device, &st))
        return rc;
    std::vector<double> s;
    if (b || sums) {
        s.resize(bh->nslots);
        HIPCHK(bh->h, hipMemcpyAsync(s.data(), bh->sums, s.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(bh->h, hipStreamSynchronize(st));
    const double dn = (double)bh->n, n4 = dn * dn * dn * dn;
    for (int t = 0; t < bh->nslots; t++) {
        if (sums)
            sums[t] = s[t];
        if (triangles)
            triangles[t] = bh->T[t];
        if (b)
            b[t] = bh->T[t] < 0.5 ? (double)NAN : bh->norm * (n4 * s[t]) / bh->T[t];
    }
    return SLICER_OK;
}

int slicer_bispectrum_spectrum(slicer_bispectrum_handle bh, double *host)
{
    if (!bh || !host)
        return fail(bh ? bh->h : nullptr, SLICER_ERR_ARG, "slicer_bispectrum_spectrum: null argument");
    if (!bh->ran)
        return fail(bh->h, SLICER_ERR_STATE, "slicer_bispectrum_spectrum before any slicer_bispectrum_run");
    return sub_read(*bh, host, bh->spec_split ? bh->spec_split : bh->spec, (size_t)bh->n * bh->H * sizeof(double2));
}

int slicer_bispectrum_read_map(slicer_bispectrum_handle bh, int32_t bin, double *host)
{
    if (!bh || !host)
        return fail(bh ? bh->h : nullptr, SLICER_ERR_ARG, "slicer_bispectrum_read_map: null argument");
    if (bin < 0 || bin >= bh->B)
        return fail(bh->h, SLICER_ERR_ARG, "slicer_bispectrum_read_map: bin = %d outside 0..%d", bin, bh->B - 1);
    if (!bh->ran)
        return fail(bh->h, SLICER_ERR_STATE, "slicer_bispectrum_read_map before any slicer_bispectrum_run");
    const size_t npix2 = (size_t)bh->n * bh->n;
    return sub_read(*bh, host, bh->F + (size_t)bin * npix2, npix2 * sizeof(double));
}

int slicer_bispectrum_destroy(slicer_bispectrum_handle bh) { return sub_destroy(bh); }
