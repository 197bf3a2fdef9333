// slicer_betti.hip -- on-device Betti numbers of a map's excursion sets as exact counts.
//
// Of an n x n f32 map x (row-major, only read) and f64 thresholds t_0 < ... < t_{T-1}, with N14's rank k(x) (the number
// of t_j <= (double)x; k(NaN) = k(-inf) = 0, k(+inf) = T) and N14's sets Q_j = {k > j}, per threshold j:
//   components[j]  the 8-connected components of Q_j (pixels joined by a side or a corner)
//   holes[j]       the 4-connected components (sides only) of the complement {k <= j}, NaN pixels included, that hold no
//                  pixel of the map's first or last row or column
//   faces[j]       the pixels with k > j (N14's number)          n_nan   the NaN pixels.
// components[j] - holes[j] is N14's vertices[j] - edges[j] + faces[j]: these are the connectivities of its closed complex.
//
// Route.  Q_j shrinks with j and the complements grow, so every connected pair meets ONCE over all thresholds:
//   k_betti_rank   ranks every pixel once into a u16 map (rank_search of slicer_rank_counts.hpp), counts the pixels of
//                  every rank and the NaNs in u32 LDS counters (2^c copies, as slicer_minkowski.hip keeps its own), one
//                  row of partial[G][T + 2] a workgroup, summed by k_column_sums into int64 count[T + 1], n_nan; sets
//                  parent[i] = i for the n^2 + 1 nodes and clears the link counters.
//   k_betti_link<SETS>, r = T ... 1: a pixel of rank exactly r is united with each of its up to 8 neighbours inside the
//                  map of rank >= r (an equal-rank pair from its larger end only); links_set[r] counts the unions that
//                  joined two trees.  After launch r the trees are the components of Q_{r-1}, so
//                  components[j] = sum over k > j of count[k] - sum over r > j of links_set[r].
//   k_betti_reset  parent[i] = i again.
//   k_betti_link<COMPLEMENT>, r = 0 ... T - 1: a pixel of rank exactly r is united with its up to 4 side neighbours of
//                  rank <= r (equal rank: from the larger end) and, in the first or last row or column, with the outside
//                  node.  After launch r the trees are the components of {k <= r} with the outside, n^2 - faces[r] + 1
//                  nodes, so holes[j] = (n^2 - faces[j] + 1) - sum over r <= j of links_c[r] - 1.
//   k_betti_finish one workgroup: the suffix and prefix sums; stores components [T], holes [T], faces [T], n_nan.
// A link launch reads count[r] first and returns at once when no pixel has rank r (no host synchronisation anywhere).
// It walks the u16 rank map eight pixels a thread (one 16-byte load) and only the pixels of rank r do more.
// Every counter and every result is rewritten by every run; nothing is carried over.
//
// Nodes.  Node 0 is the outside, pixel p (row-major) is node p + 1; n <= 32768, so ids and n^2 + 1 fit 31 bits.
//
// The union-find, and why it cannot hang.  parent[] is a u32 word a node.
//   Invariant: parent[i] <= i, and a word only ever decreases (a root's by one compare-and-swap from i to a smaller
//   index, a non-root's by atomicMin).  So a root is the smallest index of its tree, and the outside node, index 0, is
//   always a root: nothing ever writes its word.
//   find(i) follows parents while parent[i] != i.  Every step strictly lowers the index: it ends after at most i steps,
//   whatever other threads write meanwhile.  On its way it lowers a non-root's word to that node's grandparent with
//   atomicMin (path halving): the new value is smaller and lies in the same tree, so the invariant holds and sets
//   never change by it.
//   unite(a, b) finds both roots; equal: 0.  With ra > rb, old = atomicCAS(&parent[ra], ra, rb); old == ra: linked, 1.
//   Otherwise ra continues from find(old), old < ra being the value THE COMPARE-AND-SWAP ITSELF returned, never a
//   re-read of memory.  ra + rb strictly falls with every retry, so the retries are bounded by the indices, and no loop
//   anywhere waits for another thread to do something.
//   A successful compare-and-swap found ra a root, so the smallest of its tree, and rb < ra is therefore in another
//   tree: it always joins two different trees (rb need not be a root any more: the word still points into rb's tree
//   and below ra).  So the successful links of a sweep number nodes - trees, whatever the order: the counts are exact
//   and the same on every run although the union order is not.
//   Coherence: the L2 of an XCD and the L1 of a CU are not kept coherent for plain loads inside a kernel.  Every read of
//   parent[] in k_betti_link is a relaxed agent-scope atomic load and every write an agent-scope atomic; no plain access
//   to it in that kernel.  A stale value would still be a former ancestor and cost a retry, not a wrong count.  Kernel
//   boundaries order the sweeps, k_betti_rank and k_betti_reset (plain stores, no linking); no cooperative launch, no
//   grid barrier, no flags.  The rank map and the counts are written by one kernel and read by later ones: plain loads.
// Link counter: a thread counts its own links, the waves add theirs to one LDS word and the workgroup does ONE integer
// atomicAdd into links[r], and none when it linked nothing.
//
// Device memory: the u16 rank map (2 n^2 B), the u32 parents (4 (n^2 + 1) B), T thresholds, partial[G][T + 2] u32,
// T + 2 int64 sums, 2 (T + 1) u32 link counters, 3 T + 1 int64 results: about 6 GB at n = 32768.
#include <hip/hip_runtime.h>

#include "slicer_rank_counts.hpp"

namespace {

constexpr int kMaxT = SLICER_BETTI_MAX_THRESHOLDS;
constexpr int kBettiMaxNpix = SLICER_BETTI_MAX_NPIX;
constexpr int kGroup = 8;                 // pixels of a thread of k_betti_link: one 16-byte load of ranks
constexpr size_t kCopyBytes = 16 * 1024;  // LDS for the copies of the rank counters (one copy may be larger)

static_assert((int64_t)kBettiMaxNpix * kBettiMaxNpix + 1 < ((int64_t)1 << 31), "node ids fit 31 bits");
static_assert(kMaxT + 1 <= 65536, "a rank fits u16");

// log2 of the copies of the T + 1 rank counters that kCopyBytes hold, 32 at most
int lg_copies_of(int T) { return lg_copies((size_t)(T + 1) * sizeof(unsigned), kCopyBytes, 5); }

size_t rank_dyn_lds(int T) { return (size_t)T * sizeof(double) + ((((size_t)T + 1) << lg_copies_of(T)) + 1) * sizeof(unsigned); }

struct RankArgs {
    const float *x;
    const double *thr;     // [T]
    unsigned short *rank;  // [n2]
    unsigned *parent;      // [n2 + 1]
    unsigned *partial;     // [gridDim.x][T + 2]
    unsigned *links;       // [2 (T + 1)], cleared here
    unsigned n2;
    int T, lg_copies;
};

// Thread q of the grid-stride loop takes the four pixels 4 q ... 4 q + 3 of the flat map (load_quad; VEC: the map is on
// the 16-byte grid).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_betti_rank(RankArgs a)
{
    extern __shared__ double dyn[];
    const int T = a.T, nb = T + 1, tid = threadIdx.x, lg = a.lg_copies, nan_at = nb << lg;
    const unsigned copy = tid & ((1 << lg) - 1), n2 = a.n2;
    double *thr = dyn;
    unsigned *cnt = reinterpret_cast<unsigned *>(dyn + T);  // rank k, copy c: cnt[(k << lg) + c]; then the NaNs
    stage_table<kThreads>(thr, a.thr, T);
    for (int k = tid; k <= nan_at; k += kThreads)
        cnt[k] = 0u;
    if (blockIdx.x == 0) {
        for (int k = tid; k < 2 * nb; k += kThreads)
            a.links[k] = 0u;
        if (tid == 0)
            a.parent[0] = 0u;
    }
    __syncthreads();
    const unsigned nquads = (n2 + kPer - 1) / kPer;
    for (unsigned q = blockIdx.x * kThreads + tid; q < nquads; q += gridDim.x * kThreads) {
        const unsigned p0 = q * kPer, have = min((unsigned)kPer, n2 - p0);
        const float4 m = load_quad<VEC>(a.x, p0, (int)have, -INFINITY);
        const float v[kPer] = {m.x, m.y, m.z, m.w};
        unsigned n_nan = 0;
        double xd[kPer];
        int pos[kPer];
#pragma unroll
        for (int e = 0; e < kPer; e++) {
            n_nan += v[e] != v[e] ? 1u : 0u;
            xd[e] = (double)v[e];
        }
        if (n_nan)
            atomicAdd(&cnt[nan_at], n_nan);
        rank_search(thr, T, xd, pos);
        if (have == kPer) {
            *reinterpret_cast<uint2 *>(a.rank + p0) =
                make_uint2((unsigned)pos[0] | (unsigned)pos[1] << 16, (unsigned)pos[2] | (unsigned)pos[3] << 16);
            if (pos[0] == pos[1] && pos[0] == pos[2] && pos[0] == pos[3]) {
                atomicAdd(&cnt[((unsigned)pos[0] << lg) + copy], (unsigned)kPer);
            } else {
#pragma unroll
                for (int e = 0; e < kPer; e++)
                    atomicAdd(&cnt[((unsigned)pos[e] << lg) + copy], 1u);
            }
        } else {
#pragma unroll
            for (int e = 0; e < kPer; e++)
                if ((unsigned)e < have) {
                    a.rank[p0 + e] = (unsigned short)pos[e];
                    atomicAdd(&cnt[((unsigned)pos[e] << lg) + copy], 1u);
                }
        }
#pragma unroll
        for (int e = 0; e < kPer; e++)
            if ((unsigned)e < have)
                a.parent[p0 + e + 1] = p0 + e + 1;
    }
    __syncthreads();
    unsigned *out = a.partial + (size_t)blockIdx.x * (nb + 1);
    for (int k = tid; k < nb; k += kThreads)
        out[k] = fold_copies(cnt, k, lg);
    if (tid == 0)
        out[nb] = cnt[nan_at];
}

// parent[i] = i for the nodes 0 ... nodes - 1, between the two sweeps
__global__ __launch_bounds__(kThreads) void k_betti_reset(unsigned *parent, unsigned nodes)
{
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < nodes; i += gridDim.x * kThreads)
        parent[i] = i;
}

// ---- the union-find (the header comment has the argument; keep the code inside it) ----
__device__ __forceinline__ unsigned uf_load(const unsigned *parent, unsigned i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of i's tree as this thread sees it.  i falls with every turn (g < p < i), so at most i turns.
__device__ __forceinline__ unsigned uf_find(unsigned *parent, unsigned i)
{
    for (;;) {
        const unsigned p = uf_load(parent, i);
        if (p == i)
            return i;
        const unsigned g = uf_load(parent, p);
        if (g == p)
            return p;
        // i is no root (its word was p < i and words only fall); g < p is in its tree: halve the path
        (void)__hip_atomic_fetch_min(parent + i, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = g;
    }
}

// 1 iff this call joined the trees of ra's and b's nodes; ra is a root as uf_find saw it.  ra + rb falls with every turn.
__device__ __forceinline__ unsigned uf_unite_root(unsigned *parent, unsigned ra, unsigned b)
{
    unsigned rb = uf_find(parent, b);
    for (;;) {
        if (ra == rb)
            return 0u;
        if (ra < rb) {
            const unsigned t = ra;
            ra = rb, rb = t;
        }
        unsigned expected = ra;
        if (__hip_atomic_compare_exchange_strong(parent + ra, &expected, rb, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return 1u;
        ra = uf_find(parent, expected);  // expected < ra: what the compare-and-swap itself returned
    }
}

struct LinkArgs {
    const unsigned short *rank;  // [n2], read with 16-byte loads up to the next multiple of 8 (allocated)
    unsigned *parent;            // [n2 + 1]
    const int64_t *count;        // [T + 1] pixels of every rank
    unsigned *links;             // this sweep's [T + 1]
    unsigned n2;
    int n, r;
};

// One rank r of one sweep.  SETS: 8 neighbours of rank >= r; otherwise 4 side neighbours of rank <= r and the outside.
// A pair of equal rank is united from its larger index only (the other end would find the roots equal).
template <bool SETS>
__global__ __launch_bounds__(kThreads) void k_betti_link(LinkArgs a)
{
    if (a.count[a.r] == 0)
        return;  // no pixel of this rank: nothing to unite, and links[r] stays 0
    __shared__ unsigned wg_links;
    if (threadIdx.x == 0)
        wg_links = 0u;
    __syncthreads();
    const int n = a.n;
    const unsigned r = (unsigned)a.r, n2 = a.n2, ngroups = (n2 + kGroup - 1) / kGroup;
    unsigned mine = 0;
    for (unsigned g = blockIdx.x * kThreads + threadIdx.x; g < ngroups; g += gridDim.x * kThreads) {
        const uint4 w = *reinterpret_cast<const uint4 *>(a.rank + (size_t)g * kGroup);
        const unsigned word[4] = {w.x, w.y, w.z, w.w};
        unsigned hits = 0;
#pragma unroll
        for (int e = 0; e < kGroup; e++)
            hits |= (((word[e / 2] >> (e % 2 * 16)) & 0xffffu) == r ? 1u : 0u) << e;
        // (what lies past the map in the last group is never looked at)
        const unsigned have = min((unsigned)kGroup, n2 - g * kGroup);
        hits &= (1u << have) - 1u;
        while (hits) {
            const int e = __builtin_ctz(hits);
            hits &= hits - 1u;
            const unsigned p = g * kGroup + e;
            const int row = (int)(p / (unsigned)n), col = (int)(p - (unsigned)row * n);
            unsigned ra = uf_find(a.parent, p + 1);
            // the neighbour at (row + dr, col + dc), pixel q: united when its rank is on this sweep's side of r
            const auto visit = [&](int dr, int dc) {
                const int rr = row + dr, cc = col + dc;
                if (rr < 0 || rr >= n || cc < 0 || cc >= n)
                    return;
                const unsigned q = (unsigned)rr * n + cc, k = a.rank[q];
                const bool other = SETS ? k > r : k < r;
                if (other || (k == r && q < p)) {
                    const unsigned linked = uf_unite_root(a.parent, ra, q + 1);
                    mine += linked;
                    if (linked)
                        ra = uf_find(a.parent, ra);  // still p's tree; its root may have moved
                }
            };
            visit(-1, 0);
            visit(0, -1);
            visit(0, 1);
            visit(1, 0);
            if (SETS) {
                visit(-1, -1);
                visit(-1, 1);
                visit(1, -1);
                visit(1, 1);
            } else if (row == 0 || row == n - 1 || col == 0 || col == n - 1) {
                mine += uf_unite_root(a.parent, ra, 0u);
            }
        }
    }
    if (mine)
        atomicAdd(&wg_links, mine);
    __syncthreads();
    if (threadIdx.x == 0 && wg_links)
        atomicAdd(a.links + r, wg_links);
}

// One workgroup.  sums = count[T + 1], n_nan; links = links_set[T + 1], links_c[T + 1].  Three threads of three waves
// walk one running sum each through LDS (T + 1 <= 1026 steps), then res = components [T], holes [T], faces [T], n_nan.
__global__ __launch_bounds__(kThreads) void k_betti_finish(const int64_t *sums, const unsigned *links, int T, int64_t n2,
                                                           int64_t *res)
{
    __shared__ int64_t faces[kMaxT + 1], linked_set[kMaxT + 1], linked_c[kMaxT + 1];
    const int nb = T + 1, tid = threadIdx.x;
    for (int k = tid; k < nb; k += kThreads) {
        faces[k] = sums[k];
        linked_set[k] = (int64_t)links[k];
        linked_c[k] = (int64_t)links[nb + k];
    }
    __syncthreads();
    if (tid == 0) {  // faces[k] = pixels of rank >= k
        int64_t run = 0;
        for (int k = T; k >= 0; k--)
            faces[k] = run += faces[k];
    } else if (tid == 64) {  // linked_set[k] = links of the set launches r >= k
        int64_t run = 0;
        for (int k = T; k >= 0; k--)
            linked_set[k] = run += linked_set[k];
    } else if (tid == 128) {  // linked_c[k] = links of the complement launches r <= k
        int64_t run = 0;
        for (int k = 0; k <= T; k++)
            linked_c[k] = run += linked_c[k];
    }
    __syncthreads();
    for (int j = tid; j < T; j += kThreads) {
        res[j] = faces[j + 1] - linked_set[j + 1];
        res[T + j] = (n2 - faces[j + 1] + 1) - linked_c[j] - 1;
        res[2 * T + j] = faces[j + 1];
    }
    if (tid == 0)
        res[3 * T] = sums[nb];
}

const RankModule kBetti = {"slicer_betti", "slicer_betti_create", "thresholds", "fewer than 1 threshold", 1, kMaxT, kBettiMaxNpix};

}  // namespace

struct slicer_betti : RankHandle {  // table: the T thresholds
    int T = 0;
    unsigned short *rank = nullptr;
    unsigned *parent = nullptr;
    unsigned *partial = nullptr;
    int64_t *sums = nullptr;  // the column sums of `partial`
    unsigned *links = nullptr;
    int64_t *res = nullptr;
};

extern "C" {

int slicer_betti_create(slicer_handle h, int32_t npix, int32_t n_thresholds, const double *thresholds, slicer_betti_handle *out)
{
    hipStream_t st = nullptr;
    slicer_betti_handle bh = nullptr;
    int rc = rank_create(h, kBetti, npix, n_thresholds, thresholds, out, &st, &bh);
    if (!bh)
        return rc;
    const char *who = kBetti.create;
    bh->T = n_thresholds;
    const size_t n2 = (size_t)npix * npix, nC = (size_t)bh->T + 2;
    const int64_t quad_groups = (int64_t)((n2 + kPer - 1) / kPer + kThreads - 1) / kThreads;
    bh->gmax = resident_groups(rank_dyn_lds(bh->T), quad_groups, h->num_cus);
    // (the rank map up to the next multiple of kGroup pixels: k_betti_link loads whole groups)
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->rank, (n2 + kGroup - 1) / kGroup * kGroup * sizeof(unsigned short));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->parent, (n2 + 1) * sizeof(unsigned));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->partial, (size_t)bh->gmax * nC * sizeof(unsigned));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->sums, nC * sizeof(int64_t));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->links, 2 * ((size_t)bh->T + 1) * sizeof(unsigned));
    rc = bh->mem.alloc(rc, h, who, (void **)&bh->res, (3 * (size_t)bh->T + 1) * sizeof(int64_t));
    return sub_done(rank_upload(rc, *bh, kBetti, st), bh, out);
}

int slicer_betti_run_npix(slicer_betti_handle bh, const float *d_map, int32_t npix)
{
    hipStream_t st;
    if (int rc = rank_run_begin(bh, d_map, npix, kBetti, &st))
        return rc;
    const int T = bh->T;
    const unsigned n2 = (unsigned)npix * (unsigned)npix;
    // grid-stride kernels: as many workgroups as the work fills, kPerCu a CU at most
    const auto groups_for = [&](unsigned items) {
        return (unsigned)std::min<int64_t>(((int64_t)items + kThreads - 1) / kThreads,
                                           std::max(kMinGroups, kPerCu * bh->h->num_cus));
    };
    {
        ProfScope ps(bh->h, KN_BETTI_RANK);
        RankArgs a{};
        a.x = d_map;
        a.thr = bh->d_table;
        a.rank = bh->rank;
        a.parent = bh->parent;
        a.partial = bh->partial;
        a.links = bh->links;
        a.n2 = n2;
        a.T = T;
        a.lg_copies = lg_copies_of(T);
        const int G = (int)std::min<unsigned>(groups_for((n2 + kPer - 1) / kPer), (unsigned)bh->gmax);
        const size_t lds = rank_dyn_lds(T);
        if ((uintptr_t)d_map % 16 == 0)
            hipLaunchKernelGGL(k_betti_rank<true>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        else
            hipLaunchKernelGGL(k_betti_rank<false>, dim3((unsigned)G), dim3(kThreads), lds, st, a);
        HIPCHK(bh->h, hipGetLastError());
        launch_column_sums(st, bh->partial, G, T + 2, bh->sums);
        HIPCHK(bh->h, hipGetLastError());
    }
    LinkArgs l{};
    l.rank = bh->rank;
    l.parent = bh->parent;
    l.count = bh->sums;
    l.n2 = n2;
    l.n = npix;
    const unsigned GL = groups_for((n2 + kGroup - 1) / kGroup);
    {
        ProfScope ps(bh->h, KN_BETTI_LINK);  // the set sweep
        l.links = bh->links;
        for (l.r = T; l.r >= 1; l.r--)
            hipLaunchKernelGGL(k_betti_link<true>, dim3(GL), dim3(kThreads), 0, st, l);
        HIPCHK(bh->h, hipGetLastError());
    }
    {
        ProfScope ps(bh->h, KN_BETTI_LINK);  // the parents again, and the complement sweep
        hipLaunchKernelGGL(k_betti_reset, dim3(groups_for(n2 + 1)), dim3(kThreads), 0, st, bh->parent, n2 + 1);
        HIPCHK(bh->h, hipGetLastError());
        l.links = bh->links + (T + 1);
        for (l.r = 0; l.r < T; l.r++)
            hipLaunchKernelGGL(k_betti_link<false>, dim3(GL), dim3(kThreads), 0, st, l);
        HIPCHK(bh->h, hipGetLastError());
    }
    {
        ProfScope ps(bh->h, KN_BETTI_FINISH);
        hipLaunchKernelGGL(k_betti_finish, dim3(1), dim3(kThreads), 0, st, bh->sums, bh->links, T, (int64_t)n2, bh->res);
        HIPCHK(bh->h, hipGetLastError());
    }
    bh->ran = true;
    return SLICER_OK;
}

int slicer_betti_run(slicer_betti_handle bh, const float *d_map)
{
    if (int rc = rank_not_null(bh, d_map, kBetti, ""))
        return rc;
    return slicer_betti_run_npix(bh, d_map, bh->n);
}

int slicer_betti_read(slicer_betti_handle bh, int64_t *components, int64_t *holes, int64_t *faces, int64_t *n_nan)
{
    if (int rc = rank_read_begin(bh, kBetti))
        return rc;
    const size_t T = (size_t)bh->T;
    return read_slices(*bh, bh->res, {{components, T}, {holes, T}, {faces, T}, {n_nan, 1}});
}

int slicer_betti_destroy(slicer_betti_handle bh) { return sub_destroy(bh); }

}  // extern "C"
