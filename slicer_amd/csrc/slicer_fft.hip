// slicer_fft.hip -- the f64 real-to-complex transform of npix^2 maps and its inverse (slicer_fft.hpp), under the shear,
// power, bispectrum, pseudo-C_l, xi and scattering handles.
//
// One kernel, k_fft_pass, does everything: one pass of a multi-pass Stockham FFT over a batch of lines (rows or
// columns).  A workgroup gathers C lines x R points of the line into LDS (points j + r L/R, twiddled by
// W_{Ns R}^{r k}), transforms them there with radix-2/3/4/5/7/8 stages, and scatters them to j/Ns Ns R + k + q Ns.  One
// pass covers a line when it fits (R = L); longer lines take two or three passes.  The first pass of a chain may load
// through a mode and the last may store through one, which is where the pre/post-processing is fused:
//   forward rows     even n: z[m] = x[2m] + i x[2m+1] (n/2 points); odd n: z = row 2p + i row 2p+1 (n points); x is the
//                    row source (FftRows): an f32 map, or a product or modulus of two maps taken as they are loaded
//   forward columns  the r2c split of those rows (into khat's [n][n/2+1]) fused into the first column load
//   inverse columns  the column source (FftCols) fused into the first column load: the spectrum times a shear filter
//                    from the bin indices, the spectrum or ones inside a band, or |khat|^2
//   inverse rows     the c2r merge (with irfft's Hermitian projection of columns 0 and n/2) fused into the first row
//                    load; the last row pass stores into the row sink (FftSink): rounded to f32, kept in f64, left
//                    packed (gamma1), or read back packed and written as gamma1, gamma2 and |gamma|.
// Twiddles: one f64 table W_n^j = exp(-2 pi i j / n), j < n, from long-double sincos on the host.  No atomics and
// no work handed between workgroups: the results are bitwise repeatable.  variant_of: which instantiation a pass runs on.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "slicer_fft.hpp"
#include "slicer_host.hpp"

namespace {

constexpr int kThreads = 512;
constexpr int kPerThread = 16;                   // complex points a thread holds through an LDS stage
constexpr int kLdsPoints = kThreads * kPerThread;  // C * R of one workgroup (128 KiB of f64 complex, + padding)
constexpr int kColCap = kLdsPoints / 8;          // column passes: at least 8 adjacent columns (128 B) per workgroup
constexpr int kMaxLines = 64;
constexpr int kMaxStages = 16;

enum Load {
    L_COMPLEX = 0, L_REAL_EVEN, L_REAL_PAIR, L_SPLIT_EVEN, L_SPLIT_PAIR, L_FILTER, L_C2R_EVEN, L_C2R_PAIR, L_BAND,
    L_REALW_EVEN, L_REALW_PAIR, L_PROD64_EVEN, L_PROD64_PAIR, L_ABS2, L_HYPOT_EVEN, L_HYPOT_PAIR
};
enum Store { S_COMPLEX = 0, S_REAL_EVEN, S_REAL_PAIR, S_GAMMA_EVEN, S_GAMMA_PAIR, S_REAL64_EVEN, S_REAL64_PAIR };
// The instantiations of k_fft_pass.  V_PLAIN, the kernel behind the shear, deflection and power outputs, is compiled
// without the loads and stores below.  V_BAND adds L_BAND and S_REAL64_* (FFT_COLS_BAND, FFT_SINK_F64); V_PCL adds
// L_REALW_*, L_PROD64_*, L_HYPOT_*, L_ABS2 and S_REAL64_* (the pseudo-C_l, xi and scattering handles).  The split was
// made to keep V_PLAIN's registers and saves none now: compiled on 2026-10-21 (hipcc, gfx950, the Makefile's flags) all
// three report 256 VGPRs, 106 SGPRs and 72 bytes of scratch.  Merging them wants measuring; until then see variant_of.
enum Variant { V_PLAIN = 0, V_BAND, V_PCL };

struct PassArgs {
    const void *in;
    const void *in2;    // L_REALW_*: the f32 mask; L_PROD64_* and L_HYPOT_*: the second f64 map
    void *out;          // complex f64 (S_COMPLEX) or the f32 map (gamma1 for S_GAMMA_*)
    float *out2, *out3;  // S_GAMMA_*: gamma2, |gamma|
    const double2 *aux;  // S_GAMMA_*: gamma1 in f64, as its last row pass left it
    const double2 *tw;   // W_n^j, j < n
    int n, H, len;       // map side, half-spectrum width n/2+1, row-transform length (n/2 even, n odd)
    int L, R, Ns;        // this chain's length; this pass's radix; product of the earlier passes' radices
    int nlines, C, Rp;   // lines of the chain; lines per workgroup; LDS pitch of a line
    int ls_in, es_in, ls_out, es_out;  // L_COMPLEX / S_COMPLEX strides (line, element), in complex elements
    int load, store, inv, cfast;       // cfast: adjacent threads take adjacent lines (columns)
    int filt;                          // L_FILTER: SLICER_SHEAR_PHI / _GAMMA1 / _GAMMA2 / _ALPHA1 / _ALPHA2
    double phi_c;                      // L_FILTER phi: -2 / (2 pi / theta)^2
    double alpha_c;                    // L_FILTER alpha: -2 / (2 pi / theta)
    double scale;                      // S_REAL_* / S_GAMMA_* / S_REAL64_*: 1 / n^2
    double band_lo2, band_hi2;         // L_BAND: the mode is kept iff lo2 <= m2 < hi2 (<= with band_closed) and m2 != 0
    int band_closed, band_ones;        // L_BAND: band_ones = the spectrum is not read, every kept mode is 1
    int band_dc;                       // L_BAND: m2 = 0 is kept as well (if the band holds it)
    int variant;                       // unused: it only keeps the kernel's argument layout, and so its code, as it was
    int nst;
    int rad[kMaxStages];
};

__device__ inline double2 cmul(double2 a, double2 b)
{
    return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
__device__ inline double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ inline double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ inline double2 conjg(double2 a) { return make_double2(a.x, -a.y); }

// W_M^x (conjugated for the inverse), M | n, 0 <= x < M
__device__ inline double2 twid(const PassArgs &a, int x, int M)
{
    const double2 w = a.tw[(size_t)x * (a.n / M)];
    return a.inv ? conjg(w) : w;
}

template <int V>
__device__ double2 load_point(const PassArgs &a, int l, int e)
{
    const int n = a.n, H = a.H;
    if (V == V_PCL) {
        switch (a.load) {
        case L_REALW_EVEN: {  // L_REAL_EVEN of the f32 products mask * map, one rounding each
            const size_t i = (size_t)l * n + 2 * e;
            const float *k = (const float *)a.in + i, *w = (const float *)a.in2 + i;
            return make_double2((double)(w[0] * k[0]), (double)(w[1] * k[1]));
        }
        case L_REALW_PAIR: {  // L_REAL_PAIR likewise
            const size_t i = (size_t)(2 * l) * n + e;
            const float *k = (const float *)a.in + i, *w = (const float *)a.in2 + i;
            return make_double2((double)(w[0] * k[0]), 2 * l + 1 < n ? (double)(w[n] * k[n]) : 0.0);
        }
        case L_PROD64_EVEN: {  // L_REAL_EVEN of the f64 products of two f64 maps
            const size_t i = (size_t)l * n + 2 * e;
            const double *x = (const double *)a.in + i, *y = (const double *)a.in2 + i;
            return make_double2(x[0] * y[0], x[1] * y[1]);
        }
        case L_PROD64_PAIR: {
            const size_t i = (size_t)(2 * l) * n + e;
            const double *x = (const double *)a.in + i, *y = (const double *)a.in2 + i;
            return make_double2(x[0] * y[0], 2 * l + 1 < n ? x[n] * y[n] : 0.0);
        }
        case L_HYPOT_EVEN: {  // L_REAL_EVEN of sqrt(x^2 + y^2) of two f64 maps, rounded after every operation
            const size_t i = (size_t)l * n + 2 * e;
            const double *x = (const double *)a.in + i, *y = (const double *)a.in2 + i;
            return make_double2(sqrt(x[0] * x[0] + y[0] * y[0]), sqrt(x[1] * x[1] + y[1] * y[1]));
        }
        case L_HYPOT_PAIR: {
            const size_t i = (size_t)(2 * l) * n + e;
            const double *x = (const double *)a.in + i, *y = (const double *)a.in2 + i;
            return make_double2(sqrt(x[0] * x[0] + y[0] * y[0]), 2 * l + 1 < n ? sqrt(x[n] * x[n] + y[n] * y[n]) : 0.0);
        }
        case L_ABS2: {  // |khat[e][l]|^2
            const double2 s = ((const double2 *)a.in)[(size_t)e * H + l];
            return make_double2(s.x * s.x + s.y * s.y, 0.0);
        }
        default: break;
        }
    }
    if (V == V_BAND && a.load == L_BAND) {  // khat[e][l] (or 1) inside the band of the exact integer m2, 0 outside and at m2 = 0
        const double f0 = (double)(e < (n + 1) / 2 ? e : e - n), f1 = (double)l;
        const double m2 = f0 * f0 + f1 * f1;  // exact: integers below 2^28
        const bool in = (m2 != 0.0 || a.band_dc) && m2 >= a.band_lo2 && (a.band_closed ? m2 <= a.band_hi2 : m2 < a.band_hi2);
        if (!in)
            return make_double2(0.0, 0.0);
        return a.band_ones ? make_double2(1.0, 0.0) : ((const double2 *)a.in)[(size_t)e * H + l];
    }
    switch (a.load) {
    case L_REAL_EVEN: {  // row l: x[2e] + i x[2e+1]
        const float *k = (const float *)a.in + (size_t)l * n + 2 * e;
        return make_double2((double)k[0], (double)k[1]);
    }
    case L_REAL_PAIR: {  // rows 2l, 2l+1 at column e
        const float *k = (const float *)a.in + (size_t)(2 * l) * n + e;
        return make_double2((double)k[0], 2 * l + 1 < n ? (double)k[n] : 0.0);
    }
    case L_SPLIT_EVEN: {  // khat[e][l] from the n/2-point transform of row e
        const int h = n / 2;
        const double2 *T = (const double2 *)a.in + (size_t)e * h;
        const double2 z = T[l % h], zc = conjg(T[(h - l % h) % h]);
        const double2 ev = make_double2(0.5 * (z.x + zc.x), 0.5 * (z.y + zc.y));
        const double2 d = csub(z, zc);
        const double2 od = make_double2(0.5 * d.y, -0.5 * d.x);  // d / 2i
        return cadd(ev, cmul(twid(a, l, n), od));
    }
    case L_SPLIT_PAIR: {  // khat[e][l] from the n-point transform of rows (e & ~1) + i (e | 1)
        const double2 *T = (const double2 *)a.in + (size_t)(e / 2) * n;
        const double2 z = T[l], zc = conjg(T[(n - l) % n]);
        if (e % 2 == 0)
            return make_double2(0.5 * (z.x + zc.x), 0.5 * (z.y + zc.y));
        const double2 d = csub(z, zc);
        return make_double2(0.5 * d.y, -0.5 * d.x);
    }
    case L_FILTER: {  // khat[e][l] times the filter at K0 ~ fftfreq index e, K1 ~ l
        const double2 s = ((const double2 *)a.in)[(size_t)e * H + l];
        const double f0 = (double)(e < (n + 1) / 2 ? e : e - n), f1 = (double)l;
        const double k2 = f0 * f0 + f1 * f1;  // exact: integers below 2^28
        if (k2 == 0.0)
            return make_double2(0.0, 0.0);
        double g;
        if (a.filt == SLICER_SHEAR_PHI)
            g = a.phi_c / k2;
        else if (a.filt == SLICER_SHEAR_GAMMA1)
            g = (f0 * f0 - f1 * f1) / k2;
        else if (a.filt == SLICER_SHEAR_GAMMA2)
            g = 2.0 * f0 * f1 / k2;
        else {  // i K_a phihat = i g khat, g = -2 f_a / (l_f k2)
            g = a.alpha_c * (a.filt == SLICER_SHEAR_ALPHA1 ? f0 : f1) / k2;
            return make_double2(-s.y * g, s.x * g);
        }
        return make_double2(s.x * g, s.y * g);
    }
    case L_C2R_EVEN: {  // Z'[e] = (X + Y) + i W_n^-e (X - Y), X = U[l][e], Y = conj U[l][h-e]; irfft keeps Re at 0, h
        const int h = n / 2;
        const double2 *U = (const double2 *)a.in + (size_t)l * H;
        double2 x = U[e], y = conjg(U[h - e]);
        if (e == 0) {
            x.y = 0.0;
            y.y = 0.0;
        }
        const double2 o = cmul(twid(a, e, n), csub(x, y));  // a.inv: W_n^-e
        return make_double2(x.x + y.x - o.y, x.y + y.y + o.x);
    }
    case L_C2R_PAIR: {  // Hermitian extensions of rows 2l and 2l+1, packed as E_a + i E_b
        const double2 *U = (const double2 *)a.in + (size_t)(2 * l) * H;
        double2 ea, eb = make_double2(0.0, 0.0);
        const bool lo = e <= (n - 1) / 2;
        ea = lo ? U[e] : conjg(U[n - e]);
        if (2 * l + 1 < n)
            eb = lo ? U[H + e] : conjg(U[H + n - e]);
        if (e == 0) {
            ea.y = 0.0;
            eb.y = 0.0;
        }
        return make_double2(ea.x - eb.y, ea.y + eb.x);
    }
    default:
        return ((const double2 *)a.in)[(size_t)l * a.ls_in + (size_t)e * a.es_in];
    }
}

template <int V>
__device__ void store_point(const PassArgs &a, int l, int e, double2 v)
{
    const int n = a.n;
    if (V != V_PLAIN && a.store == S_REAL64_EVEN) {  // S_REAL_EVEN without the cast
        double *o = (double *)a.out + (size_t)l * n + 2 * e;
        o[0] = v.x * a.scale;
        o[1] = v.y * a.scale;
        return;
    }
    if (V != V_PLAIN && a.store == S_REAL64_PAIR) {  // S_REAL_PAIR without the cast
        double *o = (double *)a.out + (size_t)(2 * l) * n + e;
        o[0] = v.x * a.scale;
        if (2 * l + 1 < n)
            o[n] = v.y * a.scale;
        return;
    }
    switch (a.store) {
    case S_REAL_EVEN: {
        float *o = (float *)a.out + (size_t)l * n + 2 * e;
        o[0] = (float)(v.x * a.scale);
        o[1] = (float)(v.y * a.scale);
        return;
    }
    case S_REAL_PAIR: {
        float *o = (float *)a.out + (size_t)(2 * l) * n + e;
        o[0] = (float)(v.x * a.scale);
        if (2 * l + 1 < n)
            o[n] = (float)(v.y * a.scale);
        return;
    }
    case S_GAMMA_EVEN:
    case S_GAMMA_PAIR: {
        const double2 g1 = a.aux[(size_t)l * a.len + e];
        const double g1x = g1.x * a.scale, g1y = g1.y * a.scale, g2x = v.x * a.scale, g2y = v.y * a.scale;
        size_t i0, i1;  // map indices of the .x and .y halves
        bool two = true;
        if (a.store == S_GAMMA_EVEN) {
            i0 = (size_t)l * n + 2 * e;
            i1 = i0 + 1;
        } else {
            i0 = (size_t)(2 * l) * n + e;
            i1 = i0 + n;
            two = 2 * l + 1 < n;
        }
        float *o1 = (float *)a.out;
        o1[i0] = (float)g1x;
        a.out2[i0] = (float)g2x;
        a.out3[i0] = (float)sqrt(g1x * g1x + g2x * g2x);
        if (two) {
            o1[i1] = (float)g1y;
            a.out2[i1] = (float)g2y;
            a.out3[i1] = (float)sqrt(g1y * g1y + g2y * g2y);
        }
        return;
    }
    default:
        ((double2 *)a.out)[(size_t)l * a.ls_out + (size_t)e * a.es_out] = v;
    }
}

// One radix-RAD Stockham stage over the C lines of R points in LDS (line c at c * Rp), in place: every thread first
// takes its butterflies into registers, then writes them back.  C * R <= kLdsPoints.
template <int RAD>
__device__ void lds_stage(const PassArgs &a, double2 *lds, int C, int R, int Ns)
{
    constexpr int kMaxB = (kPerThread + RAD - 1) / RAD;
    const int nj = R / RAD, nb = C * nj;
    double2 w[RAD];
#pragma unroll
    for (int e = 0; e < RAD; e++)
        w[e] = twid(a, e, RAD);
    double2 v[kMaxB][RAD];
#pragma unroll
    for (int u = 0; u < kMaxB; u++) {
        const int b = threadIdx.x + u * kThreads;
        if (b < nb) {
            const int c = b / nj, j = b - c * nj, k = j % Ns;
            const double2 *p = lds + c * a.Rp + j;
#pragma unroll
            for (int q = 0; q < RAD; q++) {
                double2 x = p[q * nj];
                if (q && k)
                    x = cmul(x, twid(a, q * k, Ns * RAD));
                v[u][q] = x;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kMaxB; u++) {
        const int b = threadIdx.x + u * kThreads;
        if (b < nb) {
            const int c = b / nj, j = b - c * nj, k = j % Ns;
            double2 *p = lds + c * a.Rp + (j / Ns) * Ns * RAD + k;
#pragma unroll
            for (int m = 0; m < RAD; m++) {
                double2 y = v[u][0];
#pragma unroll
                for (int q = 1; q < RAD; q++)
                    y = cadd(y, cmul(v[u][q], w[(q * m) % RAD]));
                p[m * Ns] = y;
            }
        }
    }
    __syncthreads();
}

template <int V>
__global__ __launch_bounds__(kThreads) void k_fft_pass(PassArgs a)
{
    extern __shared__ double2 lds[];
    const int C = a.C, R = a.R, l0 = blockIdx.x * C, j = blockIdx.y, k = j % a.Ns, stride = a.L / R;
    for (int t = threadIdx.x; t < C * R; t += kThreads) {
        const int c = a.cfast ? t % C : t / R, r = a.cfast ? t / C : t % R, l = l0 + c;
        double2 v = make_double2(0.0, 0.0);
        if (l < a.nlines) {
            v = load_point<V>(a, l, j + r * stride);
            if (k && r)
                v = cmul(v, twid(a, r * k, a.Ns * R));
        }
        lds[c * a.Rp + r] = v;
    }
    __syncthreads();
    int ns = 1;
    for (int s = 0; s < a.nst; s++) {
        switch (a.rad[s]) {
        case 2: lds_stage<2>(a, lds, C, R, ns); break;
        case 3: lds_stage<3>(a, lds, C, R, ns); break;
        case 4: lds_stage<4>(a, lds, C, R, ns); break;
        case 5: lds_stage<5>(a, lds, C, R, ns); break;
        case 7: lds_stage<7>(a, lds, C, R, ns); break;
        default: lds_stage<8>(a, lds, C, R, ns); break;
        }
        ns *= a.rad[s];
    }
    const int base = (j / a.Ns) * a.Ns * R + k;
    for (int t = threadIdx.x; t < C * R; t += kThreads) {
        const int c = a.cfast ? t % C : t / R, q = a.cfast ? t / C : t % R, l = l0 + c;
        if (l < a.nlines)
            store_point<V>(a, l, base + q * a.Ns, lds[c * a.Rp + q]);
    }
}

// one pass of a chain: radix R (itself split into LDS stages), Ns, lines per workgroup
struct Pass {
    int R, Ns, C, Rp, nst;
    int rad[kMaxStages];
};

// passes of a length-L transform over nlines lines, each radix at most cap
std::vector<Pass> plan_chain(int L, int nlines, int cap)
{
    std::vector<Pass> out;
    int rem = L, ns = 1;
    do {
        int R = 1;
        for (int d = std::min(rem, cap); d >= 2; d--)
            if (rem % d == 0) {
                R = d;
                break;
            }
        if (R == 1 && rem > 1)  // cap below the smallest prime factor (only a forced split): take that factor
            for (int p : {2, 3, 5, 7})
                if (rem % p == 0) {
                    R = p;
                    break;
                }
        Pass p{};
        p.R = R;
        p.Ns = ns;
        p.C = std::max(1, std::min({kLdsPoints / std::max(R, 1), kMaxLines, nlines}));
        p.Rp = R + (R % 2 == 0);  // odd LDS pitch: the line-strided accesses of column loads spread over the banks
        int x = R;
        for (int r : {8, 4, 2, 3, 5, 7})
            while (x % r == 0) {
                p.rad[p.nst++] = r;
                x /= r;
            }
        out.push_back(p);
        rem /= R;
        ns *= R;
    } while (rem > 1);
    return out;
}

}  // namespace

// The plan (slicer_fft.hpp).  The inverse runs the chains of the forward transform backwards.
struct slicer_fft_s {
    slicer_handle h = nullptr;
    int device = 0;
    int n = 0, H = 0, len = 0, rows = 0;  // rows x len: the row transforms (n x n/2 even, ceil(n/2) x n odd)
    std::vector<Pass> row_chain, col_chain;
    double2 *tw = nullptr;
    double2 *A = nullptr, *B = nullptr, *Cb = nullptr;  // complex f64, n * H each: row output, pass intermediates
    DevAllocs mem;
};

namespace {

// Where the ends of a chain read and write, and how (see PassArgs).
struct End {
    const void *in;
    void *out;
    int load, store;
    int ls_in, es_in, ls_out, es_out;
};

// The instantiation a pass is launched on.  pcl: the transform was started from the masked, product or hypot rows or
// the |khat|^2 columns; then every pass of both its chains is V_PCL's.  Otherwise only the pass that needs V_BAND gets it.
Variant variant_of(bool pcl, int load, int store)
{
    if (pcl)
        return V_PCL;
    return load == L_BAND || store == S_REAL64_EVEN || store == S_REAL64_PAIR ? V_BAND : V_PLAIN;
}

// Launch the passes of one chain; intermediates alternate between f->B and f->Cb (neither is e.in nor e.out).
int run_chain(slicer_fft_s *f, hipStream_t st, const std::vector<Pass> &passes, bool cols, bool inv, bool pcl,
              const End &e, const PassArgs &proto)
{
    const int m = (int)passes.size();
    const int ls = cols ? 1 : f->len, es = cols ? f->H : 1;  // intermediate layout of the chain's domain
    const void *in = e.in;
    for (int p = 0; p < m; p++) {
        const Pass &ps = passes[p];
        PassArgs a = proto;
        a.tw = f->tw;
        a.n = f->n;
        a.H = f->H;
        a.len = f->len;
        a.L = cols ? f->n : f->len;
        a.nlines = cols ? f->H : f->rows;
        a.R = ps.R;
        a.Ns = ps.Ns;
        a.C = ps.C;
        a.Rp = ps.Rp;
        a.nst = ps.nst;
        for (int s = 0; s < ps.nst; s++)
            a.rad[s] = ps.rad[s];
        a.inv = inv;
        a.cfast = cols;
        a.in = in;
        a.load = p == 0 ? e.load : L_COMPLEX;
        a.ls_in = p == 0 ? e.ls_in : ls;
        a.es_in = p == 0 ? e.es_in : es;
        if (p == m - 1) {
            a.out = e.out;
            a.store = e.store;
            a.ls_out = e.ls_out;
            a.es_out = e.es_out;
        } else {
            a.out = (m - 2 - p) % 2 == 0 ? f->B : f->Cb;
            a.store = S_COMPLEX;
            a.ls_out = ls;
            a.es_out = es;
        }
        const size_t lds = (size_t)ps.C * ps.Rp * sizeof(double2);
        const dim3 grid((unsigned)((a.nlines + ps.C - 1) / ps.C), (unsigned)(a.L / ps.R));
        switch (variant_of(pcl, a.load, a.store)) {
        case V_PCL: hipLaunchKernelGGL(k_fft_pass<V_PCL>, grid, dim3(kThreads), lds, st, a); break;
        case V_BAND: hipLaunchKernelGGL(k_fft_pass<V_BAND>, grid, dim3(kThreads), lds, st, a); break;
        default: hipLaunchKernelGGL(k_fft_pass<V_PLAIN>, grid, dim3(kThreads), lds, st, a);
        }
        HIPCHK(f->h, hipGetLastError());
        in = a.out;
    }
    return SLICER_OK;
}

}  // namespace

int slicer_fft_create(slicer_handle h, int npix, int split, hipStream_t st, int device, const char *who,
                      slicer_fft_s **out)
{
    *out = nullptr;
    slicer_fft_s *f = new (std::nothrow) slicer_fft_s;
    if (!f)
        return fail(h, SLICER_ERR_NOMEM, "out of host memory");
    const int n = npix;
    f->h = h;
    f->device = device;
    f->n = n;
    f->H = n / 2 + 1;
    f->len = n % 2 == 0 ? n / 2 : n;
    f->rows = n % 2 == 0 ? n : (n + 1) / 2;
    auto cap = [&](int L, int c) { return split ? std::max(2, (int)std::floor(std::sqrt((double)L))) : c; };
    f->row_chain = plan_chain(f->len, f->rows, cap(f->len, kLdsPoints));
    f->col_chain = plan_chain(n, f->H, cap(n, kColCap));
    const size_t passes = std::max(f->row_chain.size(), f->col_chain.size());

    int rc = SLICER_OK;
    for (const void *kernel : {(const void *)k_fft_pass<V_PLAIN>, (const void *)k_fft_pass<V_BAND>,
                               (const void *)k_fft_pass<V_PCL>})
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((kLdsPoints + kMaxLines) * sizeof(double2))) != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: cannot raise the LDS limit of the FFT kernel", who);
    const size_t cbytes = (size_t)n * f->H * sizeof(double2);
    rc = f->mem.alloc(rc, h, who, (void **)&f->tw, (size_t)n * sizeof(double2));
    rc = f->mem.alloc(rc, h, who, (void **)&f->A, cbytes);
    if (passes >= 2)
        rc = f->mem.alloc(rc, h, who, (void **)&f->B, cbytes);
    if (passes >= 3)
        rc = f->mem.alloc(rc, h, who, (void **)&f->Cb, cbytes);
    if (rc == SLICER_OK) {
        std::vector<double2> tw(n);
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (int j = 0; j < n; j++) {
            const long double t = two_pi * (long double)j / (long double)n;
            tw[j] = make_double2((double)cosl(t), (double)-sinl(t));
        }
        hipError_t e = hipMemcpyAsync(f->tw, tw.data(), n * sizeof(double2), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);  // tw is a host temporary
        if (e != hipSuccess)
            rc = fail(h, SLICER_ERR_HIP, "%s: twiddle upload: %s", who, hipGetErrorString(e));
    }
    if (rc != SLICER_OK) {
        slicer_fft_destroy(f);
        return rc;
    }
    *out = f;
    return SLICER_OK;
}


int slicer_fft_r2c(slicer_fft_s *f, hipStream_t st, const FftRows &src, double2 *khat)
{
    static const int kLoad[][2] = {{L_REAL_PAIR, L_REAL_EVEN}, {L_REALW_PAIR, L_REALW_EVEN},
                                   {L_PROD64_PAIR, L_PROD64_EVEN}, {L_HYPOT_PAIR, L_HYPOT_EVEN}};  // [src.kind][even]
    const bool even = f->n % 2 == 0, pcl = src.kind != FFT_ROWS_F32;
    PassArgs p{};
    p.in2 = src.y;
    // rows of the source -> A (row layout) -> split + columns -> khat (column layout)
    End e{src.x, f->A, kLoad[src.kind][even], S_COMPLEX, 0, 0, f->len, 1};
    if (int rc = run_chain(f, st, f->row_chain, false, false, pcl, e, p))
        return rc;
    e = End{f->A, khat, even ? L_SPLIT_EVEN : L_SPLIT_PAIR, S_COMPLEX, 0, 0, 1, f->H};
    return run_chain(f, st, f->col_chain, true, false, pcl, e, p);
}

int slicer_fft_c2r(slicer_fft_s *f, hipStream_t st, const FftCols &src, const FftSink &dst)
{
    static const int kLoad[] = {L_FILTER, L_BAND, L_ABS2};  // [src.kind]
    static const int kStore[][2] = {{S_REAL_PAIR, S_REAL_EVEN}, {S_REAL64_PAIR, S_REAL64_EVEN}, {S_COMPLEX, S_COMPLEX},
                                    {S_GAMMA_PAIR, S_GAMMA_EVEN}};  // [dst.kind][even]
    const bool even = f->n % 2 == 0, pcl = src.kind == FFT_COLS_ABS2, packed = dst.kind == FFT_SINK_PACKED;
    PassArgs p{};
    p.filt = src.which;
    p.phi_c = src.phi_c;
    p.alpha_c = src.alpha_c;
    p.band_lo2 = src.lo2;
    p.band_hi2 = src.hi2;
    p.band_closed = src.closed;
    p.band_ones = src.khat == nullptr;
    p.band_dc = src.keep_dc;
    p.scale = 1.0 / ((double)f->n * (double)f->n);
    p.out2 = dst.out2;
    p.out3 = dst.out3;
    p.aux = dst.packed;
    // the source + columns khat -> A (column layout); c2r rows A -> the sink (the packed one in A's row layout)
    End e{src.khat, f->A, kLoad[src.kind], S_COMPLEX, 0, 0, 1, f->H};
    if (int rc = run_chain(f, st, f->col_chain, true, true, pcl, e, p))
        return rc;
    e = End{f->A, dst.out, even ? L_C2R_EVEN : L_C2R_PAIR, kStore[dst.kind][even], 0, 0, packed ? f->len : 0, packed};
    return run_chain(f, st, f->row_chain, false, true, pcl, e, p);
}

void slicer_fft_destroy(slicer_fft_s *f) { delete f; }
