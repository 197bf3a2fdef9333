// slicer_lensing_host.cpp -- weights of the Born-approximation convergence maps, host only.
//
// kappa_s = sum_p c_sp (m_p - <m_p>), with, for every plane p whose far edge lies in front of the source
// (z(ld2_p) <= zs + 1e-4; every other plane gets 0):
//   c_sp = 4 pi / (c^2/G) * E(zl_p, zs) * g_p * (1 + zl_p)^2 / a_p
//   zl_p   = int z chi(z) dz / int chi(z) dz over [z(ld_p), z(ld2_p)]          effective lens redshift
//   E      = D_A(zl) D_A(zl, zs) / D_A(zs) = chi_l (chi_s - chi_l) / ((1 + zl) chi_s)   (flat)
//   a_p    = (2 chi(zl_p) tan(fov / 2))^2 / npix^2                              pixel area, (Mpc/h)^2
//   g_p    = D+(zl_p) / D+(zsnap_p)                                            linear growth correction (optional)
// Background: flat w0waCDM with H0 = 100 (distances in Mpc/h), the expansion rate of the planner (planner.cpp:
// expansionRate), but chi(z) integrated to ~1e-15 instead of the planner's deliberately biased table.
#include <cmath>
#include <cstdio>
#include <vector>

#include "slicer_host.hpp"

namespace {

struct Cosmology {
    double omegaM, omegaLambda, w0, wa;  // w(a) = w0 + wa (1 - a)
};

// Physical constants (astropy's values): c (exact), G (CODATA 2018), the IAU 2015 nominal solar mass and the parsec.
constexpr double kSpeedOfLight = 299792458.0;     // m/s
constexpr double kGNewton = 6.67430e-11;          // m^3 / (kg s^2)
constexpr double kSolarMass = 1.988409870698051e30;  // kg
constexpr double kMpc = 3.0856775814913673e22;    // m
constexpr double kHubbleDistance = 2997.92458;    // c / (100 km/s/Mpc) in Mpc/h

// c^2 / G in 1e10 Msun / Mpc
double c2_over_g() { return kSpeedOfLight * kSpeedOfLight / kGNewton * (kMpc / kSolarMass) / 1e10; }

// 20-point Gauss-Legendre rule on [-1, 1] (nodes by Newton iteration on P_20)
struct GaussLegendre {
    static constexpr int kN = 20;
    double x[kN], w[kN];
    GaussLegendre()
    {
        for (int i = 0; i < kN; i++) {
            double z = cos(M_PI * (i + 0.75) / (kN + 0.5)), dp = 0;
            for (int it = 0; it < 100; it++) {
                double p0 = 1, p1 = 0;
                for (int k = 1; k <= kN; k++) {
                    const double p2 = p1;
                    p1 = p0;
                    p0 = ((2 * k - 1) * z * p1 - (k - 1) * p2) / k;
                }
                dp = kN * (z * p0 - p1) / (z * z - 1);
                const double dz = p0 / dp;
                z -= dz;
                if (fabs(dz) < 1e-16)
                    break;
            }
            x[i] = z;
            w[i] = 2 / ((1 - z * z) * dp * dp);
        }
    }
    // integral of f over [a, b] in panels no wider than `width`
    template <class F>
    double integrate(F f, double a, double b, double width) const
    {
        if (!(b > a))
            return 0;
        const int panels = (int)ceil((b - a) / width);
        const double h = (b - a) / panels;
        double total = 0;
        for (int k = 0; k < panels; k++) {
            const double lo = a + k * h, mid = lo + 0.5 * h;
            double s = 0;
            for (int i = 0; i < kN; i++)
                s += w[i] * f(mid + 0.5 * h * x[i]);
            total += 0.5 * h * s;
        }
        return total;
    }
};
const GaussLegendre kGL;
constexpr double kPanel = 0.05;  // redshift width of a quadrature panel

struct Background {
    Cosmology c;
    double E(double z) const  // H(z) / H0
    {
        const double a1 = 1.0 + z;
        const double dark = c.omegaLambda * pow(a1, 3.0 * (1.0 + c.w0 + c.wa)) * exp(-3.0 * c.wa * z / a1);
        return sqrt(dark + c.omegaM * pow(a1, 3) + (1.0 - c.omegaM - c.omegaLambda) * pow(a1, 2));
    }
    double chi(double z) const  // line-of-sight comoving distance, Mpc/h
    {
        return kHubbleDistance * kGL.integrate([&](double x) { return 1.0 / E(x); }, 0.0, z, kPanel);
    }
    double z_of_chi(double target) const  // chi is increasing and concave: Newton from below converges monotonically
    {
        if (!(target > 0))
            return 0;
        double z = target / kHubbleDistance / E(0.0);
        for (int it = 0; it < 100; it++) {
            const double dz = (target - chi(z)) * E(z) / kHubbleDistance;
            z += dz;
            if (fabs(dz) <= 1e-15 * (1 + z))
                break;
        }
        return z;
    }
    // d ln E / d ln a
    double dlnE_dlna(double a) const
    {
        const double wsum = 1.0 + c.w0 + c.wa;
        const double de = c.omegaLambda * pow(a, -3.0 * wsum) * exp(-3.0 * c.wa * (1.0 - a));
        const double ok = 1.0 - c.omegaM - c.omegaLambda;
        const double e2 = c.omegaM * pow(a, -3.0) + de + ok * pow(a, -2.0);
        const double de2 = -3.0 * c.omegaM * pow(a, -3.0) + de * (-3.0 * wsum + 3.0 * c.wa * a) - 2.0 * ok * pow(a, -2.0);
        return 0.5 * de2 / e2;
    }
    // Linear growing mode (unnormalised): D'' + (2 + dlnE/dlna) D' - 3/2 Om(a) D = 0 in x = ln a, smooth dark energy,
    // started in matter domination at a = 1e-5 with D = D' = a; classical RK4 with steps of at most 2^-10 in ln a.
    double growth(double z) const
    {
        const double x0 = log(1e-5), x1 = -log1p(z);
        const int steps = (int)ceil((x1 - x0) * 1024.0);
        const double h = (x1 - x0) / steps;
        auto rhs = [&](double x, double d, double v, double &dd, double &dv) {
            const double a = exp(x), e = E(1.0 / a - 1.0);
            dd = v;
            dv = -(2.0 + dlnE_dlna(a)) * v + 1.5 * c.omegaM * pow(a, -3.0) / (e * e) * d;
        };
        double d = exp(x0), v = exp(x0);
        for (int i = 0; i < steps; i++) {
            const double x = x0 + i * h;
            double k1d, k1v, k2d, k2v, k3d, k3v, k4d, k4v;
            rhs(x, d, v, k1d, k1v);
            rhs(x + 0.5 * h, d + 0.5 * h * k1d, v + 0.5 * h * k1v, k2d, k2v);
            rhs(x + 0.5 * h, d + 0.5 * h * k2d, v + 0.5 * h * k2v, k3d, k3v);
            rhs(x + h, d + h * k3d, v + h * k3v, k4d, k4v);
            d += h / 6.0 * (k1d + 2 * k2d + 2 * k3d + k4d);
            v += h / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v);
        }
        return d;
    }
};

int refuse(int code, const char *fmt, double a = 0, double b = 0)
{
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b);
    return fail(nullptr, code, "%s", buf);
}

// what slicer_lensing_weights and slicer_lensing_plane_strengths refuse alike; 0 if the arguments pass
int check_planes(const char *who, double omega_m, double omega_lambda, double fov_deg, int32_t npix, int32_t physical,
                 int32_t n_planes, const double *ld, const double *ld2, const double *zsnap, int32_t n_sources,
                 const double *zs, const void *out)
{
    if (physical)
        return refuse(SLICER_ERR_UNSUPPORTED, "kappa maps: a physical pixel size (one map size per plane) is not supported");
    if (fabs(1.0 - omega_m - omega_lambda) > 1e-5)
        return refuse(SLICER_ERR_UNSUPPORTED, "kappa maps need a flat background (Omega_m = %g, Omega_Lambda = %g)", omega_m,
                      omega_lambda);
    if (!(omega_m > 0) || !(fov_deg > 0 && fov_deg < 180) || npix <= 0 || n_planes <= 0 || !ld || !ld2 || !zsnap ||
        !out || n_sources <= 0 || (!zs && n_sources != n_planes))
        return fail(nullptr, SLICER_ERR_ARG, "%s: bad argument", who);
    for (int p = 0; p < n_planes; p++)
        if (!(ld[p] >= 0 && ld2[p] > ld[p]) || !(zsnap[p] >= 0)) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s: plane edges %g, %g out of order", who, ld[p], ld2[p]);
            return fail(nullptr, SLICER_ERR_ARG, "%s", buf);
        }
    return SLICER_OK;
}

// per plane: the edge redshifts, the effective lens redshift and its distance, the pixel area and the growth correction
struct PlaneGeometry {
    std::vector<double> lo, up, zl, chil, area, g;
    PlaneGeometry(const Background &bg, double fov_deg, int32_t npix, int32_t growth, int32_t n_planes, const double *ld,
                  const double *ld2, const double *zsnap)
        : lo(n_planes), up(n_planes), zl(n_planes), chil(n_planes), area(n_planes), g(n_planes)
    {
        const double side = 2.0 * tan(fov_deg * M_PI / 360.0) / npix;  // pixel side per unit distance
        for (int p = 0; p < n_planes; p++) {
            lo[p] = bg.z_of_chi(ld[p]);
            up[p] = bg.z_of_chi(ld2[p]);
            const double width = (up[p] - lo[p]) / 4;  // at least four panels per plane
            const double num = kGL.integrate([&](double z) { return z * bg.chi(z); }, lo[p], up[p], width);
            const double den = kGL.integrate([&](double z) { return bg.chi(z); }, lo[p], up[p], width);
            zl[p] = num / den;
            chil[p] = bg.chi(zl[p]);
            area[p] = (side * chil[p]) * (side * chil[p]);
            g[p] = growth ? bg.growth(zl[p]) / bg.growth(zsnap[p]) : 1.0;
        }
    }
};

}  // namespace

int slicer_lensing_weights(double omega_m, double omega_lambda, double w0, double wa, double fov_deg, int32_t npix,
                           int32_t growth, int32_t physical, int32_t n_planes, const double *ld, const double *ld2,
                           const double *zsnap, int32_t n_sources, const double *zs, double *coeff, double *zlo,
                           double *zup, double *zl, double *chil)
{
    if (int rc = check_planes("slicer_lensing_weights", omega_m, omega_lambda, fov_deg, npix, physical, n_planes, ld, ld2,
                              zsnap, n_sources, zs, coeff))
        return rc;
    const Background bg{Cosmology{omega_m, omega_lambda, w0, wa}};
    const double four_pi_g_over_c2 = 4.0 * M_PI / c2_over_g();
    const PlaneGeometry pg(bg, fov_deg, npix, growth, n_planes, ld, ld2, zsnap);
    const std::vector<double> &vlo = pg.lo, &vup = pg.up, &vzl = pg.zl, &vchil = pg.chil;
    std::vector<double> base(n_planes);
    for (int p = 0; p < n_planes; p++)
        base[p] = four_pi_g_over_c2 * pg.g[p] * (1.0 + vzl[p]) * (1.0 + vzl[p]) / pg.area[p];
    for (int s = 0; s < n_sources; s++) {
        const double z_s = zs ? zs[s] : vup[s];
        const double chi_s = bg.chi(z_s);
        for (int p = 0; p < n_planes; p++) {
            double c = 0;
            if (vup[p] <= z_s + 1e-4 && chi_s > 0) {
                const double eff = vchil[p] * (chi_s - vchil[p]) / ((1.0 + vzl[p]) * chi_s);
                c = base[p] * eff;
            }
            coeff[(size_t)s * n_planes + p] = c;
        }
    }
    for (int p = 0; p < n_planes; p++) {
        if (zlo)
            zlo[p] = vlo[p];
        if (zup)
            zup[p] = vup[p];
        if (zl)
            zl[p] = vzl[p];
        if (chil)
            chil[p] = vchil[p];
    }
    return SLICER_OK;
}

int slicer_lensing_plane_strengths(double omega_m, double omega_lambda, double w0, double wa, double fov_deg, int32_t npix,
                                   int32_t growth, int32_t physical, int32_t n_planes, const double *ld,
                                   const double *ld2, const double *zsnap, int32_t n_sources, const double *zs,
                                   double *strength, double *chil, double *chis, int32_t *n_in_front)
{
    if (int rc = check_planes("slicer_lensing_plane_strengths", omega_m, omega_lambda, fov_deg, npix, physical, n_planes, ld,
                              ld2, zsnap, n_sources, zs, strength))
        return rc;
    const Background bg{Cosmology{omega_m, omega_lambda, w0, wa}};
    const double four_pi_g_over_c2 = 4.0 * M_PI / c2_over_g();
    const PlaneGeometry pg(bg, fov_deg, npix, growth, n_planes, ld, ld2, zsnap);
    for (int p = 0; p < n_planes; p++) {
        strength[p] = four_pi_g_over_c2 * pg.g[p] * (1.0 + pg.zl[p]) * pg.chil[p] / pg.area[p];
        if (chil)
            chil[p] = pg.chil[p];
    }
    for (int s = 0; s < n_sources; s++) {
        const double z_s = zs ? zs[s] : pg.up[s];
        if (chis)
            chis[s] = bg.chi(z_s);
        if (!n_in_front)
            continue;
        n_in_front[s] = 0;
        for (int p = 0; p < n_planes; p++)
            n_in_front[s] += pg.up[p] <= z_s + 1e-4 ? 1 : 0;
    }
    return SLICER_OK;
}
