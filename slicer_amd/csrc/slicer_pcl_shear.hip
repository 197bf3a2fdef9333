// slicer_pcl_shear.hip -- on-device E/B pseudo-C_l of masked shear maps: the spin-2 rotation of the masked spectra, the
// coupled bandpowers of E, B and kappa, the spin-0, spin-2 and spin-4 coupling matrices of the mask and the block
// decoupling (the definitions are in include/slicer_amd.h).
//
// The handle is built on a cross power handle (slicer_power.hip, row N7) over its component list, and shares the mask
// and the LU of row N17 (slicer_pcl_internal.hpp); the transforms are those of slicer_fft.hip:
//   run       per component slicer_power_transform_masked, per field k_pcl2_rotate on the stored spectra of gamma1 and
//             gamma2, then slicer_power_bin_stored: once over all components (cross), or once per field over its own
//             (auto; the bandpowers are copied to the handle's table field by field)
//   set_mask  pcl_build_mask; A = irfft2(|rfft2 w|^2); M_0 column by column exactly as slicer_pcl_set_mask; then for
//             s = 2, 4: k_pcl2_weights fills the half-plane spectra (C_s, 0) and (S_s, 0), and per non-empty bin b'
//             G_c, G_s = irfft2 of them inside F_b' (slicer_fft_inverse_band, DC kept), Q_c, Q_s = rfft2(A G_c), rfft2(A G_s),
//             k_pcl2_combine turns their real parts into C_s Q_c + S_s Q_s and C_s Q_s - S_s Q_c in place, and
//             slicer_power_bin_real bins the two into column b' of M_s and X_s
//   read      the LUs of the three block systems, factorised by set_mask on the host, applied pair group by pair group
// No atomics anywhere; every element-wise kernel is a grid-stride loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "slicer_power_internal.hpp"
#include "slicer_host.hpp"
#include "slicer_pcl_internal.hpp"

namespace {

constexpr int kThreads = 256;
constexpr unsigned kMaxGroups = 1024;  // of the element-wise kernels: beyond 2^18 elements a thread takes several
constexpr int kMaxComponents = 128;  // the power handle's map limit

// (C_s, S_s) of mode (j0, j1) on a grid of side n, s = 2 or 4; one IEEE operation per step, no contraction.  On the
// Nyquist lines of an even n the sines are 0 (the mean over the aliases +n/2 and -n/2) and the cosines keep their values.
__host__ __device__ inline void spin_phase(int n, int j0, int j1, int spin, double *c, double *s)
{
    const double a = (double)j0 * (double)j0, b = (double)j1 * (double)j1, m2 = a + b;  // exact integers
    if (m2 == 0.0) {
        *c = 1.0;
        *s = 0.0;
        return;
    }
    const double c2 = (a - b) / m2, s2 = (2.0 * (double)j0 * (double)j1) / m2;
    const int aj0 = j0 < 0 ? -j0 : j0, aj1 = j1 < 0 ? -j1 : j1;
    const bool nyq = n % 2 == 0 && (aj0 == n / 2 || aj1 == n / 2);
    if (spin == 2) {
        *c = c2;
        *s = nyq ? 0.0 : s2;
        return;
    }
    const double cc = c2 * c2, ss = s2 * s2, cs = c2 * s2;
    *c = cc - ss;
    *s = nyq ? 0.0 : 2.0 * cs;
}

__host__ __device__ inline int signed_index(int n, int i0) { return i0 < (n + 1) / 2 ? i0 : i0 - n; }

// Wc = (C_s, 0), Ws = (S_s, 0) over the [n][H] half plane
__global__ __launch_bounds__(kThreads) void k_pcl2_weights(double2 *Wc, double2 *Ws, int n, int H, int spin)
{
    const size_t total = (size_t)n * H;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int i0 = (int)(i / H), i1 = (int)(i - (size_t)i0 * H);
        double c, s;
        spin_phase(n, signed_index(n, i0), i1, spin, &c, &s);
        Wc[i] = make_double2(c, 0.0);
        Ws[i] = make_double2(s, 0.0);
    }
}

// (g1, g2) <- (E, B) = (c2 g1 + s2 g2, c2 g2 - s2 g1) in place, on the real and imaginary parts separately; every
// product is rounded, then the sum
__global__ __launch_bounds__(kThreads) void k_pcl2_rotate(double2 *g1, double2 *g2, int n, int H)
{
    const size_t total = (size_t)n * H;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const int i0 = (int)(i / H), i1 = (int)(i - (size_t)i0 * H);
        double c, s;
        spin_phase(n, signed_index(n, i0), i1, 2, &c, &s);
        const double2 a = g1[i], b = g2[i];
        g1[i] = make_double2(c * a.x + s * b.x, c * a.y + s * b.y);
        g2[i] = make_double2(c * b.x - s * a.x, c * b.y - s * a.y);
    }
}

// (Re Qc, Re Qs) <- (C Re Qc + S Re Qs, C Re Qs - S Re Qc) in place, the imaginary parts 0; C, S the real parts of Wc, Ws
__global__ __launch_bounds__(kThreads) void k_pcl2_combine(double2 *Qc, double2 *Qs, const double2 *Wc,
                                                           const double2 *Ws, size_t total)
{
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const double c = Wc[i].x, s = Ws[i].x, qc = Qc[i].x, qs = Qs[i].x;
        Qc[i] = make_double2(c * qc + s * qs, 0.0);
        Qs[i] = make_double2(c * qs - s * qc, 0.0);
    }
}

unsigned groups_for(size_t total) { return (unsigned)std::min<size_t>(kMaxGroups, (total + kThreads - 1) / kThreads); }

// index of the pair (i, j), i <= j, among S components: slicer_power_create's order
inline int pair_of(int i, int j, int S)
{
    if (i > j)
        std::swap(i, j);
    return i * S - i * (i - 1) / 2 + (j - i);
}

enum { M0 = 0, M2, X2, M4, X4, kMatrices };

}  // namespace

struct slicer_pcl2_s : SubHandle {
    slicer_power_handle pw = nullptr;  // cross, over all components (cross) or over one field's (auto)
    int n = 0, H = 0, F = 0, kappa = 0, cross = 0, B = 0;
    int ncf = 0;     // components per field: E, B and kappa if present
    int npf = 0;     // pairs within a field
    int npairs = 0;  // rows of the bandpower tables
    std::vector<double> e2;
    std::vector<int64_t> counts;
    std::vector<int> active;
    std::vector<double> M[kMatrices];              // [B][B] each
    std::vector<double> lu0, lu2, lu4;             // the LUs of the active systems: na, 2 na and 4 na square
    std::vector<int> piv0, piv2, piv4;
    double mean_w = 0.0, mean_w2 = 0.0;
    float *w = nullptr;
    double *A = nullptr, *Gc = nullptr, *Gs = nullptr, *f = nullptr;
    double *Mt = nullptr;  // [kMatrices][b'][b], as the columns are binned
    double *cl = nullptr;  // auto mode: the coupled bandpowers [F * npf][B]
    double2 *Qc = nullptr, *Qs = nullptr, *Wc = nullptr, *Ws = nullptr, *partial = nullptr;
    unsigned long long *bad = nullptr;
    bool has_mask = false, ran = false;
    SLICER_FFT_INTERNAL ~slicer_pcl2_s()
    {
        if (pw)
            slicer_power_destroy(pw);
    }
};

int slicer_pcl2_phases(int32_t npix, int32_t spin, double *C, double *S)
{
    if (npix < 2 || !C || !S)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl2_phases: npix below 2, or null output");
    if (spin != 2 && spin != 4)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl2_phases: spin = %d, expected 2 or 4", spin);
    const int n = npix, H = n / 2 + 1;
    for (int i0 = 0; i0 < n; i0++)
        for (int i1 = 0; i1 < H; i1++)
            spin_phase(n, signed_index(n, i0), i1, spin, &C[(size_t)i0 * H + i1], &S[(size_t)i0 * H + i1]);
    return SLICER_OK;
}

int slicer_pcl2_create(slicer_handle h, int32_t npix, double angle_deg, int32_t n_fields, int32_t with_kappa,
                       int32_t cross, int32_t n_edges, const double *edges, slicer_pcl2_handle *out)
{
    const char *who = "slicer_pcl2_create";
    if (!h || !out)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_create: null argument");
    *out = nullptr;
    if (!edges)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_create: the edges are required");
    if (n_edges - 1 > SLICER_PCL2_MAX_BINS)
        return fail(h, SLICER_ERR_UNSUPPORTED, "slicer_pcl2_create: %d bins, at most %d", n_edges - 1, SLICER_PCL2_MAX_BINS);
    if (with_kappa != 0 && with_kappa != 1)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_create: with_kappa = %d, expected 0 or 1", with_kappa);
    if (cross != 0 && cross != 1)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_create: cross = %d, expected 0 or 1", cross);
    const int ncf = 2 + with_kappa;
    if (n_fields < 1 || n_fields > kMaxComponents / ncf)
        return fail(h, SLICER_ERR_UNSUPPORTED, "slicer_pcl2_create: n_fields = %d outside 1..%d", n_fields,
                    kMaxComponents / ncf);
    slicer_power_handle pw = nullptr;
    if (int rc = slicer_power_create(h, npix, angle_deg, cross ? n_fields * ncf : ncf, 1, n_edges, edges, &pw)) {
        // the refusals of slicer_power_create under this call's name
        std::string why = slicer_last_error(h);
        const std::string pre = "slicer_power_create";
        if (why.compare(0, pre.size(), pre) == 0)
            why = who + why.substr(pre.size());
        return fail(h, rc, "%s", why.c_str());
    }
    hipStream_t st = nullptr;
    slicer_pcl2_handle ph = nullptr;
    if (int rc = sub_new(h, who, &st, &ph)) {
        slicer_power_destroy(pw);
        return rc;
    }
    const int n = npix, H = n / 2 + 1, B = n_edges - 1;
    ph->pw = pw;
    ph->n = n;
    ph->H = H;
    ph->F = n_fields;
    ph->kappa = with_kappa;
    ph->cross = cross;
    ph->B = B;
    ph->ncf = ncf;
    ph->npf = ncf * (ncf + 1) / 2;
    const int nc = n_fields * ncf;
    ph->npairs = cross ? nc * (nc + 1) / 2 : n_fields * ph->npf;
    ph->e2.resize(B + 1);
    for (int b = 0; b <= B; b++)
        ph->e2[b] = edges[b] * edges[b];
    ph->counts.resize(B);
    std::vector<double> mean(B);
    int rc = slicer_power_bins(n, n_edges, edges, ph->counts.data(), mean.data());
    for (int b = 0; b < B; b++)
        if (ph->counts[b] > 0)
            ph->active.push_back(b);
    const size_t px = (size_t)n * n, hp = (size_t)n * H;
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->w, px * sizeof(float));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->A, px * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Gc, px * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Gs, px * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Qc, hp * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Qs, hp * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Wc, hp * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Ws, hp * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->f, (size_t)n * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->Mt, (size_t)kMatrices * B * B * sizeof(double), &st);
    if (!cross)
        rc = ph->mem.alloc(rc, h, who, (void **)&ph->cl, (size_t)ph->npairs * B * sizeof(double));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->partial, kPclMomentGroups * sizeof(double2));
    rc = ph->mem.alloc(rc, h, who, (void **)&ph->bad, kPclMomentGroups * sizeof(unsigned long long));
    return sub_done(rc, ph, out);
}

int slicer_pcl2_set_mask(slicer_pcl2_handle ph, const float *d_mask, double taper_width_pix)
{
    const char *who = "slicer_pcl2_set_mask";
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl2_set_mask: null handle");
    slicer_handle h = ph->h;
    if (!std::isfinite(taper_width_pix) || taper_width_pix < 0.0)
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_set_mask: the taper width must be finite and not negative");
    if (!d_mask && !(taper_width_pix > 0.0))
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_set_mask: neither a mask nor a taper");
    hipStream_t st;
    if (int rc = sub_stream(h, ph->device, &st))
        return rc;
    ph->has_mask = ph->ran = false;
    const int n = ph->n, H = ph->H, B = ph->B;
    if (int rc = pcl_build_mask(h, who, st, n, d_mask, taper_width_pix, ph->w, ph->f, ph->partial, ph->bad, &ph->mean_w,
                                &ph->mean_w2))
        return rc;

    // A, then the matrices column by column: M_0 as row N17 computes its M, then spin 2 and spin 4
    slicer_fft_s *plan = slicer_power_plan(ph->pw);
    if (int rc = slicer_fft_forward(plan, st, ph->w, ph->Qc))
        return rc;
    if (int rc = slicer_fft_inverse_abs2(plan, st, ph->Qc, ph->A))
        return rc;
    const double norm = 1.0 / ((double)n * (double)n);
    const size_t hp = (size_t)n * H, BB = (size_t)B * B;
    for (int b : ph->active) {
        if (int rc = slicer_fft_inverse_band(plan, st, nullptr, ph->e2[b], ph->e2[b + 1], b == B - 1, ph->Gc, 1))
            return rc;
        if (int rc = slicer_fft_forward_product(plan, st, ph->A, ph->Gc, ph->Qc))
            return rc;
        if (int rc = slicer_power_bin_real(ph->pw, st, ph->Qc, norm, b, ph->Mt + M0 * BB))
            return rc;
    }
    for (int k = 0; k < 2; k++) {
        double *dM = ph->Mt + (k ? M4 : M2) * BB, *dX = ph->Mt + (k ? X4 : X2) * BB;
        hipLaunchKernelGGL(k_pcl2_weights, dim3(groups_for(hp)), dim3(kThreads), 0, st, ph->Wc, ph->Ws, n, H, k ? 4 : 2);
        HIPCHK(h, hipGetLastError());
        for (int b : ph->active) {
            const int closed = b == B - 1;
            if (int rc = slicer_fft_inverse_band(plan, st, ph->Wc, ph->e2[b], ph->e2[b + 1], closed, ph->Gc, 1))
                return rc;
            if (int rc = slicer_fft_inverse_band(plan, st, ph->Ws, ph->e2[b], ph->e2[b + 1], closed, ph->Gs, 1))
                return rc;
            if (int rc = slicer_fft_forward_product(plan, st, ph->A, ph->Gc, ph->Qc))
                return rc;
            if (int rc = slicer_fft_forward_product(plan, st, ph->A, ph->Gs, ph->Qs))
                return rc;
            hipLaunchKernelGGL(k_pcl2_combine, dim3(groups_for(hp)), dim3(kThreads), 0, st, ph->Qc, ph->Qs, ph->Wc,
                               ph->Ws, hp);
            HIPCHK(h, hipGetLastError());
            if (int rc = slicer_power_bin_real(ph->pw, st, ph->Qc, norm, b, dM))
                return rc;
            if (int rc = slicer_power_bin_real(ph->pw, st, ph->Qs, norm, b, dX))
                return rc;
        }
    }
    std::vector<double> Mt(kMatrices * BB);
    HIPCHK(h, hipMemcpyAsync(Mt.data(), ph->Mt, Mt.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int m = 0; m < kMatrices; m++) {
        ph->M[m].assign(BB, 0.0);
        for (int b : ph->active)
            for (int c : ph->active)
                ph->M[m][(size_t)b * B + c] = Mt[m * BB + (size_t)c * B + b];
    }

    // the three systems on the active bins: M_0; [[M_2, -X_2], [X_2, M_2]]; the 4 x 4 blocks of P, R and T
    const int na = (int)ph->active.size();
    auto at = [&](int m, int i, int j) { return ph->M[m][(size_t)ph->active[i] * B + ph->active[j]]; };
    ph->lu0.resize((size_t)na * na);
    ph->lu2.resize((size_t)4 * na * na);
    ph->lu4.resize((size_t)16 * na * na);
    for (int i = 0; i < na; i++)
        for (int j = 0; j < na; j++) {
            ph->lu0[(size_t)i * na + j] = at(M0, i, j);
            const double m2 = at(M2, i, j), x2 = at(X2, i, j);
            const double blk2[2][2] = {{m2, -x2}, {x2, m2}};
            for (int r = 0; r < 2; r++)
                for (int c = 0; c < 2; c++)
                    ph->lu2[(size_t)(r * na + i) * (2 * na) + (c * na + j)] = blk2[r][c];
            const double P = (at(M0, i, j) + at(M4, i, j)) / 2.0, R = (at(M0, i, j) - at(M4, i, j)) / 2.0,
                         T = at(X4, i, j) / 2.0;
            const double blk4[4][4] = {{P, -T, -T, R}, {T, P, -R, -T}, {T, -R, P, -T}, {R, T, T, P}};
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++)
                    ph->lu4[(size_t)(r * na + i) * (4 * na) + (c * na + j)] = blk4[r][c];
        }
    if (!lu_factor(ph->lu0, na, ph->piv0) || !lu_factor(ph->lu2, 2 * na, ph->piv2) ||
        !lu_factor(ph->lu4, 4 * na, ph->piv4))
        return fail(h, SLICER_ERR_ARG, "slicer_pcl2_set_mask: coupling matrix singular");
    ph->has_mask = true;
    return SLICER_OK;
}

int slicer_pcl2_read_mask(slicer_pcl2_handle ph, float *host)
{
    if (!ph || !host)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl2_read_mask: null argument");
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_read_mask before any slicer_pcl2_set_mask");
    return sub_read(*ph, host, ph->w, (size_t)ph->n * ph->n * sizeof(float));
}

int slicer_pcl2_coupling(slicer_pcl2_handle ph, double *m0, double *m2, double *x2, double *m4, double *x4,
                         double *mean_w, double *mean_w2)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl2_coupling: null handle");
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_coupling before any slicer_pcl2_set_mask");
    double *dst[kMatrices] = {m0, m2, x2, m4, x4};
    for (int m = 0; m < kMatrices; m++)
        if (dst[m])
            std::copy(ph->M[m].begin(), ph->M[m].end(), dst[m]);
    if (mean_w)
        *mean_w = ph->mean_w;
    if (mean_w2)
        *mean_w2 = ph->mean_w2;
    return SLICER_OK;
}

int slicer_pcl2_run(slicer_pcl2_handle ph, const float *const *d_maps)
{
    if (!ph || !d_maps)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl2_run: null argument");
    const int ncf = ph->ncf;
    for (int s = 0; s < ph->F * ncf; s++)
        if (!d_maps[s])
            return fail(ph->h, SLICER_ERR_ARG, "slicer_pcl2_run: map %d is null", s);
    if (!ph->has_mask)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_run before any slicer_pcl2_set_mask");
    hipStream_t st;
    if (int rc = sub_stream(ph->h, ph->device, &st))
        return rc;
    ph->ran = false;
    const size_t hp = (size_t)ph->n * ph->H;
    for (int f = 0; f < ph->F; f++) {
        const int slot0 = ph->cross ? f * ncf : 0;
        for (int c = 0; c < ncf; c++)
            if (int rc = slicer_power_transform_masked(ph->pw, st, slot0 + c, d_maps[f * ncf + c], ph->w))
                return rc;
        hipLaunchKernelGGL(k_pcl2_rotate, dim3(groups_for(hp)), dim3(kThreads), 0, st, slicer_power_stored(ph->pw, slot0),
                           slicer_power_stored(ph->pw, slot0 + 1), ph->n, ph->H);
        HIPCHK(ph->h, hipGetLastError());
        if (!ph->cross)
            if (int rc = slicer_power_bin_stored(ph->pw, st, ph->cl + (size_t)f * ph->npf * ph->B))
                return rc;
    }
    if (ph->cross)
        if (int rc = slicer_power_bin_stored(ph->pw, st, nullptr))
            return rc;
    ph->ran = true;
    return SLICER_OK;
}

int slicer_pcl2_spectrum(slicer_pcl2_handle ph, int32_t field, int32_t comp, double *host)
{
    if (!ph || !host)
        return fail(ph ? ph->h : nullptr, SLICER_ERR_ARG, "slicer_pcl2_spectrum: null argument");
    if (field < 0 || field >= ph->F)
        return fail(ph->h, SLICER_ERR_ARG, "slicer_pcl2_spectrum: field = %d outside 0..%d", field, ph->F - 1);
    if (comp < 0 || comp >= ph->ncf)
        return fail(ph->h, SLICER_ERR_ARG, "slicer_pcl2_spectrum: comp = %d outside 0..%d", comp, ph->ncf - 1);
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_spectrum before any slicer_pcl2_run");
    if (!ph->cross && field != ph->F - 1)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_spectrum: auto mode keeps only the last field's spectra");
    return slicer_power_spectrum(ph->pw, (ph->cross ? field * ph->ncf : 0) + comp, host);
}

int slicer_pcl2_read(slicer_pcl2_handle ph, double *cl, double *coupled, double *ell_mean, int64_t *counts)
{
    if (!ph)
        return fail(nullptr, SLICER_ERR_ARG, "slicer_pcl2_read: null handle");
    if (!ph->ran)
        return fail(ph->h, SLICER_ERR_STATE, "slicer_pcl2_read before any slicer_pcl2_run");
    const int B = ph->B, na = (int)ph->active.size(), ncf = ph->ncf;
    std::vector<double> own;
    double *ct = coupled;
    if (cl && !ct) {
        own.resize((size_t)ph->npairs * B);
        ct = own.data();
    }
    if (ph->cross) {
        if (int rc = slicer_power_read(ph->pw, ct, ell_mean, counts))
            return rc;
    } else {
        hipStream_t st;
        if (int rc = sub_stream(ph->h, ph->device, &st))
            return rc;
        if (ct)
            HIPCHK(ph->h, hipMemcpyAsync(ct, ph->cl, (size_t)ph->npairs * B * sizeof(double), hipMemcpyDeviceToHost, st));
        if (int rc = slicer_power_read(ph->pw, nullptr, ell_mean, counts))  // waits for the stream
            return rc;
    }
    if (!cl)
        return SLICER_OK;
    for (size_t i = 0; i < (size_t)ph->npairs * B; i++)
        cl[i] = NAN;
    // row of the pair (component a of field f, component b of field g) in the tables
    auto row = [&](int f, int a, int g, int b) {
        if (ph->cross)
            return pair_of(f * ncf + a, g * ncf + b, ph->F * ncf);
        return f * ph->npf + pair_of(a, b, ncf);  // f == g
    };
    // one block system over `m` rows of the tables: gather the active bins, solve, scatter
    std::vector<double> x((size_t)4 * na);
    auto solve = [&](const std::vector<double> &lu, const std::vector<int> &piv, const int *rows, int m) {
        for (int r = 0; r < m; r++)
            for (int i = 0; i < na; i++)
                x[(size_t)r * na + i] = ct[(size_t)rows[r] * B + ph->active[i]];
        lu_solve(lu, m * na, piv, x.data());
        for (int r = m - 1; r >= 0; r--)  // for f = g the BE row is the EB row: EB's own solution is the one kept
            for (int i = 0; i < na; i++)
                cl[(size_t)rows[r] * B + ph->active[i]] = x[(size_t)r * na + i];
    };
    enum { E = 0, Bm = 1, K = 2 };
    for (int f = 0; f < ph->F; f++)
        for (int g = f; g < (ph->cross ? ph->F : f + 1); g++) {
            const int r4[4] = {row(f, E, g, E), row(f, E, g, Bm), row(f, Bm, g, E), row(f, Bm, g, Bm)};
            solve(ph->lu4, ph->piv4, r4, 4);
            if (!ph->kappa)
                continue;
            const int r2[2] = {row(f, K, g, E), row(f, K, g, Bm)};
            solve(ph->lu2, ph->piv2, r2, 2);
            if (g != f) {
                const int q2[2] = {row(g, K, f, E), row(g, K, f, Bm)};
                solve(ph->lu2, ph->piv2, q2, 2);
            }
            const int r1[1] = {row(f, K, g, K)};
            solve(ph->lu0, ph->piv0, r1, 1);
        }
    return SLICER_OK;
}

int slicer_pcl2_destroy(slicer_pcl2_handle ph) { return sub_destroy(ph); }
