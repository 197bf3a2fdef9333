// driver_lensing.cpp -- the lensing outputs of SLICER_amd.  All are opt-in, need --kappa and are computed on device 0;
// without --kappa the run is unchanged.  The per-source files carry the kappa file's name with another token, and its header.
//   * --kappa all|z1,z2,...: Born convergence maps, one FITS per source redshift, accumulated from the finalized total
//     maps of every pass (the reference's post-processing script Lens/kslicer.py);
//     --kappa-no-growth drops its linear-growth correction.
//   * --shear: per source the shear maps gamma1, gamma2, |gamma| and the lensing potential phi of the kappa map (the
//     reference's Lens/smr.py).
//   * --deflection (with --shear): the deflection maps .alpha1_z, .alpha2_z.  --shear-derivative fft|gradient (with
//     --shear or --raytrace, default fft) chooses where the gammas and alphas come from: the FFT filters, or smr's
//     derivative="gradient", finite differences of phi that do not wrap the map's edges.  The
//     phi and kappa files are the same either way.
//   * --raytrace: one ray per pixel through the planes, near to far.  Every plane's lens map
//     strength_p (m_p - mean m_p) is turned into its deflection, convergence and shear maps (the device work of --shear
//     --deflection, per plane) and the rays step through them at chi(zl_p).  Per source .rt_kappa_z, .rt_gamma1_z,
//     .rt_gamma2_z, .rt_omega_z (the distortion matrix) and .rt_alpha1_z, .rt_alpha2_z (the total deflection, radians).
//   * --power auto|cross: <directory><simulation>.cl_<npix>_<suffix>.txt, the binned auto (or auto and cross) power
//     spectra C_l of the kappa maps (Lens/smr.py's PS without its defects); --power-edges r0,r1,...
//     sets the bin edges in units of l_f = 2 pi / ANGLE (default 0, 1, ..., npix-1).
//   * --pcl auto|cross with --pcl-edges r0,r1,... (required; at most 513 edges in the units of --power-edges) and at
//     least one of --pcl-taper ARCMIN (a border taper of that width, ARCMIN npix / (60 ANGLE) pixels) and --pcl-mask
//     FILE.fits (an image of the maps' size, BITPIX -32 or -64): <directory><simulation>.pcl_<npix>_<suffix>.txt, the
//     masked pseudo-C_l of the kappa maps, the layout of the .cl_ file with '#' lines for the mask (mean_w, mean_w2,
//     taper_arcmin, taper_pix, mask) and per pair the decoupled bandpower C_s_t followed by the coupled one Ct_s_t; and
//     .pclm_<npix>_<suffix>.txt, the mode-coupling matrix M, one row per line.
//   * --pcl-shear (with --pcl and --shear; at most 129 edges): the E/B pseudo-C_l of every source's (gamma1, gamma2) as
//     they are written, with its kappa map, under --pcl's mask, edges and mode: .pcleb_<npix>_<suffix>.txt, the '#'
//     lines and the bin columns of the .pcl_ file, then for the sources s <= t (cross; s = t with auto) the decoupled
//     and the coupled bandpowers C_EE_s_t Ct_EE_s_t, and likewise EB, BE (s < t only: BE_s_s is EB_s_s), BB, kE, kB and,
//     for s < t, kE_t_s and kB_t_s (XY_s_t: component X of source s against Y of source t; kk is in the .pcl_ file);
//     and .pclebm_<npix>_<suffix>.txt, the coupling matrices M0, M2, X2, M4, X4 one after another, each under a
//     '# <name>' line, one row per line.
//   * --xi auto|cross with --xi-edges a0,a1,... (required; at most 513 edges in arcminutes, one arcminute being
//     npix / (60 ANGLE) pixels) and optionally --xi-mask FILE.fits (an image of the maps' size, BITPIX -32 or -64, finite
//     and >= 0: the weight map shared by all maps): <directory><simulation>.xi_<npix>_<suffix>.txt, the real-space
//     two-point functions xi_kk of the kappa maps (auto, or every pair with cross): '#' lines (npix, angle, the source
//     redshifts, mask, the padded size P, the column names), then per bin r_lo r_hi r_mean (arcminutes), xi of every
//     pair, the pair weight W_b and the pair count N_b; nan marks an empty bin.  With --shear also .xipm_<npix>_<suffix>
//     .txt, xi+ and xi- of every source's (gamma1, gamma2) as they are written, auto only.  The maps do not wrap, and
//     the mask is divided out exactly.  Refused for physical runs.
//   * --moments: <directory><simulation>.moments_<npix>_<suffix>.txt, the raw central power sums S_2 ... S_8 and the
//     mean of every kappa map and of --moments-levels L (default 0) successive 2x2 block means of it, about each level's
//     own mean (Lens/moment.py and Lens/halve.py).
//   * --peaks lo,hi,bins: <directory><simulation>.peaks_<npix>_<suffix>.txt, the one-point PDF histogram of every kappa
//     map and the counts of its peaks and minima by height (strictly above / below all 8 neighbours; the map does not
//     wrap) over `bins` (1 ... 1024) uniform bins from lo to hi; with --moments also of every level of its pyramid of
//     block means.
//   * --minkowski lo,hi,bins: <directory><simulation>.minkowski_<npix>_<suffix>.txt, the Minkowski functionals of the
//     excursion sets kappa >= t of every kappa map as exact counts of the faces, edges and vertices of the pixel complex
//     (area, outline length inside the field and on the rim, Euler characteristic) over the bins + 1 thresholds that are
//     the edges of `bins` (1 ... 1024) uniform bins from lo to hi; with --moments also of every level of its pyramid of
//     block means; with --smooth and / or --shape-noise also .smooth_minkowski_, .noisy_minkowski_ and
//     .noisy_smooth_minkowski_, where --peaks writes its tables of those maps.
//   * --betti lo,hi,bins: <directory><simulation>.betti_<npix>_<suffix>.txt, the Betti numbers of the same excursion
//     sets over the same kind of thresholds as exact counts: per threshold the 8-connected components of the set and its
//     holes (the 4-connected components of the complement that do not touch the map's rim), whose difference is
//     --minkowski's euler; the levels and the tables .smooth_betti_, .noisy_betti_ and .noisy_smooth_betti_ as for
//     --minkowski.  The Betti tables are the last files of a run.
//   * --bispectrum all|equilateral with --bispectrum-edges r0,r1,... (required; 2 ... 33 edges in the units of
//     --power-edges): <directory><simulation>.bl_<npix>_<suffix>.txt, the binned bispectrum B_ijk of every kappa map over
//     all triples i <= j <= k of the bins or over the equilateral ones, with the number of closed triangles of every
//     triple; nan marks a triple without one.  The smoothed and the noisy maps have none.
//   * --smooth gauss|map:a1,a2,...: per source and per scale a_k (arcminutes; sigma = a_k npix / (60 ANGLE) pixels)
//     the kappa map smoothed with a Gaussian truncated at 4 sigma (gauss) or turned into the aperture mass of the filter
//     built from it (map), .<kind><k>_kappa_z..., with the kappa file's header and the keys SCALE (arcminutes) and RADIUS
//     (the filter's reach in pixels: the rim of a map file that saw a truncated aperture).  With --moments and / or
//     --peaks also .smooth_moments_ and .smooth_peaks_: the tables above of every smoothed map and of its pyramid, with
//     a leading column `scale` = k.
//   * --shape-noise sigma_e,ngal[,seed[,nreal]]: per source and per realisation r = 0 ... nreal-1 (1 ... 1024, default 1)
//     the kappa map plus white Gaussian shape noise of sigma_pix = sigma_e / sqrt(ngal A_pix) a pixel (sigma_e per
//     ellipticity component, ngal per arcmin^2, A_pix the pixel's area in arcmin^2), .noisy<r>_kappa_z..., with the kappa
//     file's header and the keys SIGMAE, NGAL, SIGMAPIX, SEED, REALIS.  The noise is a pure function of (seed, the
//     source's rank in ascending redshift, r, pixel): counter-based, so the same on every run, rank count and order of
//     the --kappa list.  With --moments and / or --peaks also .noisy_moments_ and .noisy_peaks_ (a leading column
//     `real`).  With --smooth every scale of the NOISY map, .noisy<r>_<kind><k>_kappa_z..., with the keys above, SCALE,
//     RADIUS and NOISESIG = sigma_pix times the filter's gain on white noise (the sigma that signal-to-noise heights are
//     in units of), and the tables .noisy_smooth_moments_ and .noisy_smooth_peaks_ (leading columns `real scale`, a
//     '# noise_sigma' line of the per-scale NOISESIG).  Refused for physical runs, whose pixels have no angle (DESIGN.md
//     S8 row N13).
//   * --starlet J:lo,hi,bins: per source the starlet transform of the kappa map (the isotropic undecimated wavelet
//     transform, B3-spline, mirrored edges) into J (1 ... 12) wavelet maps .starlet<j>_kappa_z..., j = 1 ... J, and the
//     coarse map .starlet0_kappa_z..., with the kappa file's header and the keys SCALE (j) and GAIN (the rms of that
//     map for white noise of unit variance a pixel, 17 digits).  Two tables of the scales j = 1 ... J over `bins`
//     (1 ... 1024) uniform bins from lo to hi: .starlet_peaks_, the histogram and the peak and minimum counts of --peaks
//     per scale, and .starlet_l1_, per bin the pixel count and the sum of |w_j| (the starlet l1-norm); rows -1, bins,
//     bins + 1 as in the --peaks table.  Without --shape-noise lo and hi are in units of kappa and all scales share the
//     edges; with it they are signal-to-noise: scale j has the edges e_b sigma_j, sigma_j = sigma_pix GAIN_j (a
//     '# sigma_scale' line), and per realisation r the same maps of the noisy map, .noisy<r>_starlet<j>_kappa_z...
//     with the keys of the noisy file first, and the tables .noisy_starlet_peaks_ and .noisy_starlet_l1_ (a leading
//     column `real`).  Refused for physical runs.
//   * --scattering J,L: <directory><simulation>.scattering_<npix>_<suffix>.txt, the wavelet scattering coefficients of
//     every kappa map over J (1 ... 12, 2^J <= npix) dyadic scales and L (1 ... 16) orientations of Morlet filters, the
//     map taken as periodic: '#' lines (npix, angle, J, L, the filter constants sigma0, xi0 and slant of
//     sigma = sigma0 2^j, xi = xi0 2^-j, s = slant / L, the column names), then per source the rows
//     z order j1 l1 j2 l2 value power (%.17g): order 0, one row, the mean and the mean square of kappa; order 1, per
//     (j1, l1), s1 and p1, the mean and the mean square of |kappa * psi_{j1 l1}|; order 2, per (j1, l1, j2 > j1, l2),
//     s2, the mean of ||kappa * psi_{j1 l1}| * psi_{j2 l2}| (power: nan); an index a row does not have is -1.  With
//     --shape-noise also .noisy_scattering_ of every noisy realisation (a leading column `real`).  Not for the pyramid
//     levels or the smoothed maps: the transform has its own scales.  npix must be a size the f64 transform takes;
//     refused for physical runs.  The scattering tables are the last files of a run without --catalogue (DESIGN.md S8
//     row N20).
//   * --catalogue min_peak[,capacity]: <directory><simulation>.catalogue_<npix>_<suffix>.txt, the peaks of every kappa
//     map (strictly above all 8 neighbours, as --peaks counts them) whose value is >= min_peak (-inf: all of them), in
//     ascending row * npix + col, at most `capacity` (1 ... 2^29; 1048576 where it is not given) of a map: '#' lines
//     (npix, angle, min_peak, capacity, the column names), then per map a line '# map z [real] [scale] n_peaks stored'
//     with the exact number of such peaks and the number listed, and one row per listed peak:
//     z [real] [scale] row col value dy dx off_row_deg off_col_deg flags (%.17g): (dy, dx) the sub-pixel offset of a
//     quadratic fit to the 3 x 3 window, (0, 0) and flags = 2 where it was not accepted; off_row_deg =
//     (((row + dy) + 0.5) / npix - 0.5) angle_deg, the angle from the field's centre, and likewise along the columns.
//     A map with more peaks than the capacity is announced on stderr and in a '# overflow' line; the run goes on.  With
//     --smooth and --shape-noise also .smooth_catalogue_, .noisy_catalogue_ and .noisy_smooth_catalogue_ (columns
//     `scale`, `real`, `real scale` after z), the maps of which --peaks writes its tables; not for pyramid levels.
//     Refused for physical runs and for npix above 32768.  The catalogue tables are the last files of a run (DESIGN.md
//     S8 row N22).
#include "driver_lensing.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <iostream>
#include <numeric>

using std::cerr;
using std::cout;
using std::endl;
using std::string;
using std::vector;

namespace slicer_amd {

constexpr double kSmoothTruncate = 4.0;  // --smooth: the filters reach to 4 sigma

string plane_label(int pll)
{
    char b[16];
    snprintf(b, sizeof b, "%03d", pll);
    return b;
}

vector<string> split(const string &s)
{
    vector<string> out;
    size_t i = 0;
    for (size_t j; (j = s.find(',', i)) != string::npos; i = j + 1)
        out.push_back(s.substr(i, j - i));
    out.push_back(s.substr(i));
    return out;
}

static int bad(const string &message)
{
    cerr << message << endl;
    return 2;
}

// printf onto the end of `text`
__attribute__((format(printf, 2, 3))) static void add(string &text, const char *fmt, ...)
{
    char piece[512];  // (the longest is a histogram row: nine numbers)
    va_list a;
    va_start(a, fmt);
    vsnprintf(piece, sizeof piece, fmt, a);
    va_end(a);
    text += piece;
}

// the whole of `token` as a double: false for an empty token and for one with anything after the number
static bool whole_double(const string &token, double *v)
{
    char *end = nullptr;
    *v = strtod(token.c_str(), &end);
    return !token.empty() && *end == '\0';
}

// a comma-separated list of doubles onto the end of `out`: false at the first piece that is not one
static bool parse_doubles(const char *value, vector<double> &out)
{
    for (const string &tok : split(value)) {
        double v;
        if (!whole_double(tok, &v))
            return false;
        out.push_back(v);
    }
    return true;
}

// The value lo,hi,bins of `option` into the bins + 1 uniform edges of slicer_peaks_edges: 0, or 2 after the message
static int uniform_edges(const string &option, const char *value, const char *meaning, vector<double> &edges)
{
    const vector<string> tok = value ? split(value) : vector<string>{};
    double lo = 0.0, hi = 0.0;
    char *end = nullptr;
    const bool three = tok.size() == 3 && whole_double(tok[0], &lo) && whole_double(tok[1], &hi) && !tok[2].empty();
    const long bins = three ? strtol(tok[2].c_str(), &end, 10) : 0;
    if (!three || *end != '\0' || bins < 1 || bins > SLICER_PEAKS_MAX_BINS)
        return bad("bad " + option + " (lo,hi,bins: " + meaning + " and the number of bins, 1 ... " +
                   std::to_string(SLICER_PEAKS_MAX_BINS) + ")");
    edges.resize(bins + 1);
    if (slicer_peaks_edges(lo, hi, (int32_t)bins, edges.data()) != SLICER_OK)
        return bad("bad " + option + ": " + slicer_last_error(nullptr));
    return 0;
}

int LensingOptions::parse(int argc, char **argv, int &i)
{
    const string a = argv[i];
    const bool has_value = i + 1 < argc;
    if (a == "--kappa" && has_value) kappa = argv[++i];
    else if (a == "--kappa-no-growth") growth = false;
    else if (a == "--shear") shear = true;
    else if (a == "--deflection") deflection = true;
    else if (a == "--raytrace") raytrace = true;
    else if (a == "--shear-derivative" && has_value) shear_derivative = argv[++i];
    else if (a == "--power" && has_value) power = argv[++i];
    else if (a == "--power-edges" && has_value) {
        if (!parse_doubles(argv[++i], power_edges))
            return bad("bad --power-edges (a comma-separated list of radii in units of l_f)");
    } else if (a == "--pcl" && has_value) pcl = argv[++i];
    else if (a == "--pcl-edges" && has_value) {
        if (!parse_doubles(argv[++i], pcl_edges))
            return bad("bad --pcl-edges (a comma-separated list of radii in units of l_f)");
        if (pcl_edges.size() > SLICER_PCL_MAX_BINS + 1)
            return bad("bad --pcl-edges (" + std::to_string(pcl_edges.size()) + " edges, at most " +
                       std::to_string(SLICER_PCL_MAX_BINS + 1) + ")");
    } else if (a == "--pcl-taper" && has_value) {
        if (!whole_double(argv[++i], &pcl_taper_arcmin) || !std::isfinite(pcl_taper_arcmin) || !(pcl_taper_arcmin > 0))
            return bad("bad --pcl-taper (the width of the border taper in arcminutes, positive)");
        pcl_taper_given = true;
    } else if (a == "--pcl-mask" && has_value) pcl_mask = argv[++i];
    else if (a == "--pcl-shear") pcl_shear = true;
    else if (a == "--xi" && has_value) xi = argv[++i];
    else if (a == "--xi-edges" && has_value) {
        if (!parse_doubles(argv[++i], xi_edges))
            return bad("bad --xi-edges (a comma-separated list of radii in arcminutes)");
        if (xi_edges.size() > SLICER_XI_MAX_BINS + 1)
            return bad("bad --xi-edges (" + std::to_string(xi_edges.size()) + " edges, at most " +
                       std::to_string(SLICER_XI_MAX_BINS + 1) + ")");
    } else if (a == "--xi-mask" && has_value) xi_mask = argv[++i];
    else if (a == "--bispectrum" && has_value) bispectrum = argv[++i];
    else if (a == "--bispectrum-edges" && has_value) {
        if (!parse_doubles(argv[++i], bispectrum_edges))
            return bad("bad --bispectrum-edges (a comma-separated list of radii in units of l_f)");
        if (bispectrum_edges.size() > SLICER_BISPECTRUM_MAX_BINS + 1)
            return bad("bad --bispectrum-edges (" + std::to_string(bispectrum_edges.size()) + " edges, at most " +
                       std::to_string(SLICER_BISPECTRUM_MAX_BINS + 1) + ")");
    } else if (a == "--moments") moments = true;
    else if (a == "--moments-levels") {
        if (!has_value)
            return bad("--moments-levels needs a value (the number of halvings below the kappa map)");
        char *end = nullptr;
        const long v = strtol(argv[++i], &end, 10);
        if (end == argv[i] || *end != '\0' || v < -1000 || v > 1000)
            return bad("bad --moments-levels (the number of halvings below the kappa map)");
        moments_levels = (int)v;
        moments_levels_given = true;
    } else if (a == "--peaks") {
        if (const int rc = uniform_edges(a, has_value ? argv[++i] : nullptr, "the first and the last edge", peaks_edges))
            return rc;
    } else if (a == "--minkowski") {
        if (const int rc = uniform_edges(a, has_value ? argv[++i] : nullptr, "the first and the last threshold",
                                         minkowski_thresholds))
            return rc;
    } else if (a == "--betti") {
        if (const int rc = uniform_edges(a, has_value ? argv[++i] : nullptr, "the first and the last threshold", betti_thresholds))
            return rc;
    } else if (a == "--smooth") {
        const string v = has_value ? argv[++i] : "";
        const size_t colon = v.find(':');
        smooth_kind = v.substr(0, colon);
        smooth_arcmin.clear();
        for (const string &tok : colon == string::npos ? vector<string>{} : split(v.substr(colon + 1))) {
            smooth_arcmin.push_back(0.0);
            if (!whole_double(tok, &smooth_arcmin.back()) || !std::isfinite(smooth_arcmin.back()) || !(smooth_arcmin.back() > 0))
                smooth_arcmin.clear();
            if (smooth_arcmin.empty())
                break;
        }
        if ((smooth_kind != "gauss" && smooth_kind != "map") || smooth_arcmin.empty())
            return bad("bad --smooth (gauss:a1,a2,... or map:a1,a2,...: positive scales in arcminutes)");
    } else if (a == "--shape-noise") {
        const vector<string> tok = has_value ? split(argv[++i]) : vector<string>{};
        const char *usage = "bad --shape-noise (sigma_e,ngal[,seed[,nreal]]: the ellipticity dispersion per component and the "
                            "galaxies per arcmin^2, both positive; seed 0 ... 2^63-1; nreal 1 ... 1024)";
        if (tok.size() < 2 || tok.size() > 4)
            return bad(usage);
        for (const string &t : tok)
            if (t.empty() || t[0] == '-' || t[0] == '+' || isspace((unsigned char)t[0]))
                return bad(usage);
        char *e2 = nullptr, *e3 = nullptr;
        const bool sigma_whole = whole_double(tok[0], &noise_sigma_e), ngal_whole = whole_double(tok[1], &noise_ngal);
        errno = 0;
        const unsigned long long seed = tok.size() > 2 ? strtoull(tok[2].c_str(), &e2, 10) : 0;
        const bool seed_ok = tok.size() <= 2 || (*e2 == '\0' && errno == 0 && seed <= (unsigned long long)INT64_MAX);
        const long nreal = tok.size() > 3 ? strtol(tok[3].c_str(), &e3, 10) : 1;
        if (!sigma_whole || !ngal_whole || !seed_ok || (tok.size() > 3 && *e3 != '\0') || nreal < 1 || nreal > 1024 ||
            !std::isfinite(noise_sigma_e) || !(noise_sigma_e > 0) || !std::isfinite(noise_ngal) || !(noise_ngal > 0))
            return bad(usage);
        noise_seed = seed;
        noise_nreal = (int)nreal;
        shape_noise = true;
    } else if (a == "--starlet") {
        const string v = has_value ? argv[++i] : "";
        const size_t colon = v.find(':');
        const string scales = v.substr(0, colon);
        char *end = nullptr;
        const long J = strtol(scales.c_str(), &end, 10);
        if (colon == string::npos || scales.empty() || isspace((unsigned char)scales[0]) || *end != '\0' || J < 1 ||
            J > SLICER_STARLET_MAX_SCALES)
            return bad("bad --starlet (J:lo,hi,bins: the number of scales, 1 ... " + std::to_string(SLICER_STARLET_MAX_SCALES) +
                       ", then the first and the last edge and the number of bins)");
        starlet_edges.clear();
        if (const int rc = uniform_edges(a, v.c_str() + colon + 1, "after J: the first and the last edge", starlet_edges))
            return rc;
        starlet_scales = (int)J;
    } else if (a == "--scattering") {
        const vector<string> tok = has_value ? split(argv[++i]) : vector<string>{};
        char *e0 = nullptr, *e1 = nullptr;
        const bool two = tok.size() == 2 && !tok[0].empty() && !tok[1].empty() && !isspace((unsigned char)tok[0][0]) &&
                         !isspace((unsigned char)tok[1][0]);
        const long J = two ? strtol(tok[0].c_str(), &e0, 10) : 0, L = two ? strtol(tok[1].c_str(), &e1, 10) : 0;
        if (!two || *e0 != '\0' || *e1 != '\0' || J < 1 || J > SLICER_SCATTERING_MAX_J || L < 1 || L > SLICER_SCATTERING_MAX_L)
            return bad("bad --scattering (J,L: the number of scales, 1 ... " + std::to_string(SLICER_SCATTERING_MAX_J) +
                       ", and of orientations, 1 ... " + std::to_string(SLICER_SCATTERING_MAX_L) + ")");
        scattering_J = (int)J;
        scattering_L = (int)L;
    } else if (a == "--catalogue") {
        const vector<string> tok = has_value ? split(argv[++i]) : vector<string>{};
        char *end = nullptr;
        const bool shaped = (tok.size() == 1 || tok.size() == 2) && whole_double(tok[0], &catalogue_min_peak) &&
                            !std::isnan(catalogue_min_peak) && (tok.size() == 1 || (!tok[1].empty() && !isspace((unsigned char)tok[1][0])));
        const long long capacity = shaped && tok.size() == 2 ? strtoll(tok[1].c_str(), &end, 10) : catalogue_capacity;
        if (!shaped || (end && *end != '\0') || capacity < 1 || capacity > SLICER_CATALOGUE_MAX_CAPACITY)
            return bad("bad --catalogue (min_peak[,capacity]: the lowest peak to list, -inf for all of them, and the most "
                       "records of a map, 1 ... " + std::to_string(SLICER_CATALOGUE_MAX_CAPACITY) + ")");
        catalogue_capacity = capacity;
        catalogue = true;
    } else
        return -1;
    return 0;
}

int LensingOptions::check() const
{
    const bool no_kappa = kappa.empty(), derivative = !shear_derivative.empty(), pw = !power.empty();
    const bool bs = !bispectrum.empty(), pc = !pcl.empty(), x = !xi.empty();
    const std::pair<bool, const char *> rules[] = {
        {shear && no_kappa, "--shear needs --kappa (the shear maps are computed from the kappa maps)"},
        {raytrace && no_kappa, "--raytrace needs --kappa (the rays are observed at the source redshifts of the kappa maps)"},
        {deflection && !shear, "--deflection needs --shear (the deflection maps are computed from the spectrum of the shear maps)"},
        {derivative && shear_derivative != "fft" && !gradient(), "bad --shear-derivative (fft or gradient)"},
        {derivative && !shear && !raytrace, "--shear-derivative needs --shear"},
        {pw && power != "auto" && power != "cross", "bad --power (auto or cross)"},
        {pw && no_kappa, "--power needs --kappa (the power spectra are those of the kappa maps)"},
        {!power_edges.empty() && !pw, "--power-edges needs --power"},
        {pc && pcl != "auto" && pcl != "cross", "bad --pcl (auto or cross)"},
        {pc && no_kappa, "--pcl needs --kappa (the pseudo-spectra are those of the kappa maps)"},
        {!pcl_edges.empty() && !pc, "--pcl-edges needs --pcl"},
        {pcl_taper_given && !pc, "--pcl-taper needs --pcl"},
        {!pcl_mask.empty() && !pc, "--pcl-mask needs --pcl"},
        {pc && pcl_edges.empty(), "--pcl needs --pcl-edges (the bin edges in units of l_f)"},
        {pc && !pcl_taper_given && pcl_mask.empty(), "--pcl needs --pcl-taper or --pcl-mask (or both)"},
        {pcl_shear && !pc, "--pcl-shear needs --pcl (the mask, the edges and the mode are those of --pcl)"},
        {pcl_shear && !shear, "--pcl-shear needs --shear (the fields are the shear maps of the sources)"},
        {x && xi != "auto" && xi != "cross", "bad --xi (auto or cross)"},
        {x && no_kappa, "--xi needs --kappa (the correlation functions are those of the kappa maps)"},
        {!xi_edges.empty() && !x, "--xi-edges needs --xi"},
        {!xi_mask.empty() && !x, "--xi-mask needs --xi"},
        {x && xi_edges.empty(), "--xi needs --xi-edges (the bin edges in arcminutes)"},
        {bs && bispectrum != "all" && bispectrum != "equilateral", "bad --bispectrum (all or equilateral)"},
        {bs && no_kappa, "--bispectrum needs --kappa (the bispectra are those of the kappa maps)"},
        {!bispectrum_edges.empty() && !bs, "--bispectrum-edges needs --bispectrum"},
        {bs && bispectrum_edges.empty(), "--bispectrum needs --bispectrum-edges (the bin edges in units of l_f)"},
        {moments && no_kappa, "--moments needs --kappa (the moments are those of the kappa maps)"},
        {moments_levels_given && !moments, "--moments-levels needs --moments"},
        {!peaks_edges.empty() && no_kappa, "--peaks needs --kappa (the histograms and peak counts are those of the kappa maps)"},
        {!minkowski_thresholds.empty() && no_kappa,
         "--minkowski needs --kappa (the Minkowski functionals are those of the kappa maps)"},
        {!betti_thresholds.empty() && no_kappa, "--betti needs --kappa (the Betti numbers are those of the kappa maps)"},
        {!smooth_kind.empty() && no_kappa, "--smooth needs --kappa (the smoothed maps are those of the kappa maps)"},
        {shape_noise && no_kappa, "--shape-noise needs --kappa (the noise is added to the kappa maps)"},
        {starlet_scales > 0 && no_kappa, "--starlet needs --kappa (the transform is that of the kappa maps)"},
        {scattering_J > 0 && no_kappa, "--scattering needs --kappa (the coefficients are those of the kappa maps)"},
        {catalogue && no_kappa, "--catalogue needs --kappa (the peaks are those of the kappa maps)"},
    };
    for (const auto &[broken, message] : rules)
        if (broken)
            return bad(message);
    if (pcl_shear && pcl_edges.size() > SLICER_PCL2_MAX_BINS + 1)
        return bad("--pcl-shear: " + std::to_string(pcl_edges.size()) + " edges in --pcl-edges, at most " +
                   std::to_string(SLICER_PCL2_MAX_BINS + 1));
    return 0;
}

int LensingOptions::check_npix(const InputParams &p) const
{
    const string npix = "npix = " + std::to_string(p.npix);
    const string fft_sizes = " is not supported (2 ... 16384, prime factors 2, 3, 5, 7 only)";
    if (shear && !slicer_shear_supported(p.npix))
        return bad("--shear: " + npix + fft_sizes);
    if (raytrace && !p.physical && !slicer_shear_supported(p.npix))  // (physical: refused with the weights)
        return bad("--raytrace: " + npix + fft_sizes);
    if (gradient() && p.npix < 5)
        return bad("--shear-derivative gradient: " + npix + " is not supported (the stencils take at least 5)");
    if (!power.empty() && !slicer_shear_supported(p.npix))
        return bad("--power: " + npix + fft_sizes);
    if (!power.empty()) {  // the edges
        const int ne = n_power_edges(p.npix);
        vector<int64_t> cnt(std::max(ne - 1, 1));
        vector<double> mr(cnt.size());
        if (slicer_power_bins(p.npix, ne, power_edges_or_null(), cnt.data(), mr.data()) != SLICER_OK)
            return bad(string("--power-edges: ") + slicer_last_error(nullptr));
    }
    if (!pcl.empty() && !slicer_shear_supported(p.npix))
        return bad("--pcl: " + npix + fft_sizes);
    if (!pcl.empty()) {  // the edges, the taper, the mask file
        vector<int64_t> cnt(std::max<size_t>(pcl_edges.size(), 2) - 1);
        vector<double> mr(cnt.size());
        if (slicer_power_bins(p.npix, (int)pcl_edges.size(), pcl_edges.data(), cnt.data(), mr.data()) != SLICER_OK)
            return bad(string("--pcl-edges: ") + slicer_last_error(nullptr));
        if (pcl_taper_given && p.physical)
            return bad("--pcl-taper: the width is an angle, and the maps of a physical run have none");
        vector<double> f(p.npix);
        if (pcl_taper_given && slicer_pcl_taper(p.npix, pcl_taper_pix(p.npix, p.fov), f.data()) != SLICER_OK)
            return bad("--pcl-taper: " + npix + ": " + slicer_last_error(nullptr));
        vector<float> w((size_t)p.npix * (size_t)p.npix);
        const string why = pcl_mask.empty() ? "" : fits_read_mask(pcl_mask, p.npix, w.data());
        if (!why.empty())
            return bad("--pcl-mask: " + why);
    }
    if (!xi.empty()) {  // the edges, the mask file
        if (p.physical)
            return bad("--xi-edges: the edges are angles, and the maps of a physical run have none");
        const vector<double> e = xi_edges_pix(p.npix, p.fov);
        if (slicer_xi_bins(p.npix, (int)e.size(), e.data(), nullptr, nullptr, nullptr) != SLICER_OK)
            return bad(string("--xi-edges: ") + slicer_last_error(nullptr));
        vector<float> w((size_t)p.npix * (size_t)p.npix);
        const string why = xi_mask.empty() ? "" : fits_read_mask(xi_mask, p.npix, w.data());
        if (!why.empty())
            return bad("--xi-mask: " + why);
    }
    if (!bispectrum.empty() && !slicer_shear_supported(p.npix))
        return bad("--bispectrum: " + npix + fft_sizes);
    if (!bispectrum.empty()) {  // the edges
        vector<int64_t> cnt(std::max<size_t>(bispectrum_edges.size(), 2) - 1);
        vector<double> mr(cnt.size());
        if (slicer_power_bins(p.npix, (int)bispectrum_edges.size(), bispectrum_edges.data(), cnt.data(), mr.data()) != SLICER_OK)
            return bad(string("--bispectrum-edges: ") + slicer_last_error(nullptr));
    }
    if (moments) {  // the pyramid's depth
        int most = 0;
        while (p.npix >> (most + 1) > 0)
            most++;
        if (p.npix < 1 || moments_levels < 0 || moments_levels > most)
            return bad("--moments-levels " + std::to_string(moments_levels) + " is outside 0 ... " + std::to_string(most) +
                       " = floor(log2 npix) for " + npix);
    }
    if (!smooth_kind.empty() && p.physical)
        return bad("--smooth: the scales are angles, and the maps of a physical run have none");
    for (size_t k = 0; k < smooth_arcmin.size(); k++)  // the radius of every scale
        if (slicer_smooth_weights(smooth_sigma_pix(k, p.npix, p.fov), kSmoothTruncate, nullptr, nullptr, nullptr) != SLICER_OK)
            return bad("--smooth: scale " + std::to_string(k) + " for " + npix + ": " + slicer_last_error(nullptr));
    if (shape_noise && p.physical)
        return bad("--shape-noise: the galaxy density is per angle, and the pixels of a physical run have none");
    if (starlet_scales > 0 && p.physical)
        return bad("--starlet: the scales are read as angles, and the maps of a physical run have none");
    if (scattering_J > 0 && p.physical)
        return bad("--scattering: the table is that of maps with an angle, and the maps of a physical run have none");
    if (scattering_J > 0 && !slicer_shear_supported(p.npix))
        return bad("--scattering: " + npix + fft_sizes);
    if (scattering_J > 0 && (1L << scattering_J) > p.npix)
        return bad("--scattering: 2^J = " + std::to_string(1L << scattering_J) + " is above " + npix);
    if (catalogue && p.physical)
        return bad("--catalogue: the offsets are angles, and the maps of a physical run have none");
    if (catalogue && p.npix > SLICER_CATALOGUE_MAX_NPIX)
        return bad("--catalogue: " + npix + " is above " + std::to_string(SLICER_CATALOGUE_MAX_NPIX));
    double sigma_pix = 0.0;
    if (shape_noise && slicer_noise_sigma_pix(noise_sigma_e, noise_ngal, p.fov, p.npix, &sigma_pix) != SLICER_OK)
        return bad("--shape-noise: " + npix + ": " + slicer_last_error(nullptr));
    return 0;
}

int plan_lensing(const LensingOptions &o, const InputParams &p, const Header &simdata, const Lens &lens, LensingPlan &plan)
{
    if (o.kappa.empty())
        return 0;
    const bool all = o.kappa == "all";  // otherwise z1,z2,...
    for (const string &tok : all ? vector<string>{} : split(o.kappa)) {
        plan.zs.push_back(0.0);
        if (!whole_double(tok, &plan.zs.back()) || !(plan.zs.back() >= 0))
            return bad("bad --kappa (all, or a comma-separated list of source redshifts)");
    }
    const int P = lens.nplanes, S = all ? P : (int)plan.zs.size();
    vector<double> zup(P);
    plan.coeff.assign((size_t)S * P, 0.0);
    if (slicer_lensing_weights(simdata.om0, simdata.oml, p.w, 0.0, p.fov, p.npix, o.growth, p.physical, P, lens.ld.data(),
                               lens.ld2.data(), lens.zfromsnap.data(), S, all ? nullptr : plan.zs.data(),
                               plan.coeff.data(), nullptr, zup.data(), nullptr, nullptr) != SLICER_OK)
        return fail(nullptr, "slicer_amd: --kappa");
    if (all)
        plan.zs = zup;
    if (!o.raytrace)
        return 0;
    plan.strength.resize(P);
    plan.chil.resize(P);
    plan.chis.resize(S);
    plan.in_front.resize(S);
    if (slicer_lensing_plane_strengths(simdata.om0, simdata.oml, p.w, 0.0, p.fov, p.npix, o.growth, p.physical, P,
                                       lens.ld.data(), lens.ld2.data(), lens.zfromsnap.data(), S, plan.zs.data(),
                                       plan.strength.data(), plan.chil.data(), plan.chis.data(),
                                       plan.in_front.data()) != SLICER_OK)
        return fail(nullptr, "slicer_amd: --raytrace");
    for (int i = 1; i < P; i++)
        if (!(plan.chil[i] > plan.chil[i - 1])) {
            cerr << "--raytrace: the plane distances are not strictly ascending (plane " << i << " at " << plan.chil[i]
                 << " after " << plan.chil[i - 1] << " Mpc/h)" << endl;
            return 2;
        }
    return 0;
}

int LensingOutputs::create()
{
    const vector<double> &zs = plan.zs;
    if (zs.empty())
        return 0;
    map.resize((size_t)p.npix * (size_t)p.npix);
    if (slicer_kappa_create(h, p.npix, (int)zs.size(), kh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --kappa");
    if ((o.shear || o.raytrace) && slicer_shear_create(h, p.npix, p.fov, shh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --shear");
    if (!o.power.empty() && zs.size() > 128) {
        cerr << "slicer_amd: --power: " << zs.size() << " sources, at most 128" << endl;
        return 2;
    }
    if (!o.power.empty() && slicer_power_create(h, p.npix, p.fov, (int)zs.size(), o.power == "cross", o.n_power_edges(p.npix),
                                                o.power_edges_or_null(), ph.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --power");
    if (!o.pcl.empty() && zs.size() > 128) {
        cerr << "slicer_amd: --pcl: " << zs.size() << " sources, at most 128" << endl;
        return 2;
    }
    if (!o.pcl.empty() && slicer_pcl_create(h, p.npix, p.fov, (int)zs.size(), o.pcl == "cross", (int)o.pcl_edges.size(),
                                            o.pcl_edges.data(), pclh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --pcl");
    if (o.pcl_shear && zs.size() > 42) {
        cerr << "slicer_amd: --pcl-shear: " << zs.size() << " sources, at most 42" << endl;
        return 2;
    }
    if (o.pcl_shear) {
        if (slicer_pcl2_create(h, p.npix, p.fov, (int)zs.size(), 1, o.pcl == "cross", (int)o.pcl_edges.size(),
                               o.pcl_edges.data(), pcl2h.out()) != SLICER_OK)
            return fail(h, "slicer_amd: --pcl-shear");
        for (size_t k = 0; k < 2 * zs.size(); k++)
            if (!pcl2_gamma.add(p.npix))
                return fail(h, "slicer_amd: --pcl-shear");
    }
    if (!o.xi.empty()) {
        const char *who = "slicer_amd: --xi";
        const vector<double> e = o.xi_edges_pix(p.npix, p.fov);
        if (slicer_xi_create(h, p.npix, 0, (int)zs.size(), o.xi == "cross", (int)e.size(), e.data(), xih.out()) != SLICER_OK ||
            (o.shear && slicer_xi_create(h, p.npix, 2, 1, 0, (int)e.size(), e.data(), xipmh.out()) != SLICER_OK))
            return fail(h, who);
        if (!o.xi_mask.empty()) {
            vector<float> w(map.size());
            DeviceMaps mask(h);
            const string why = fits_read_mask(o.xi_mask, p.npix, w.data());
            if (!why.empty()) {
                cerr << who << "-mask: " << why << endl;
                return 1;
            }
            // (slicer_xi_set_weights waits for the stream: neither copy of the mask is read after it returns)
            if (!mask.add(p.npix) || slicer_copy_to_device(h, mask.maps[0], w.data(), w.size() * sizeof(float)) != SLICER_OK ||
                slicer_xi_set_weights(xih, mask.maps[0]) != SLICER_OK ||
                (xipmh && slicer_xi_set_weights(xipmh, mask.maps[0]) != SLICER_OK))
                return fail(h, who);
        }
    }
    if (o.moments && slicer_moments_create(h, p.npix, o.moments_levels, SLICER_HALVE_MEAN, mh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --moments");
    if (!o.peaks_edges.empty() &&
        slicer_peaks_create(h, p.npix, (int)o.peaks_edges.size(), o.peaks_edges.data(), pkh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --peaks");
    if (!o.minkowski_thresholds.empty() &&
        slicer_minkowski_create(h, p.npix, (int)o.minkowski_thresholds.size(), o.minkowski_thresholds.data(), mkh.out()) !=
            SLICER_OK)
        return fail(h, "slicer_amd: --minkowski");
    if (!o.betti_thresholds.empty() &&
        slicer_betti_create(h, p.npix, (int)o.betti_thresholds.size(), o.betti_thresholds.data(), bth.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --betti");
    if (o.catalogue && slicer_catalogue_create(h, p.npix, o.catalogue_capacity, nullptr, cth.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --catalogue");
    if (!o.bispectrum.empty()) {
        const int B = (int)o.bispectrum_edges.size() - 1;
        for (int i = 0; i < B; i++)
            for (int j = i; j < B; j++)
                for (int k = j; k < B; k++)
                    if (o.bispectrum == "all" || (i == j && j == k))
                        bispectrum_triples.insert(bispectrum_triples.end(), {i, j, k});
        if (slicer_bispectrum_create(h, p.npix, p.fov, B + 1, o.bispectrum_edges.data(), (int)bispectrum_triples.size() / 3,
                                     bispectrum_triples.data(), bsh.out()) != SLICER_OK)
            return fail(h, "slicer_amd: --bispectrum");
    }
    for (size_t k = 0; k < o.smooth_arcmin.size(); k++) {
        const double sigma = o.smooth_sigma_pix(k, p.npix, p.fov);
        smooth_radius.push_back(0);
        if (slicer_smooth_weights(sigma, kSmoothTruncate, &smooth_radius.back(), nullptr, nullptr) != SLICER_OK ||
            slicer_smooth_create(h, p.npix, o.smooth_kind == "map" ? SLICER_SMOOTH_MAP : SLICER_SMOOTH_GAUSS, sigma,
                                 kSmoothTruncate, smh.emplace_back().out()) != SLICER_OK)
            return fail(h, "slicer_amd: --smooth");
    }
    if (o.shape_noise) {
        if (slicer_noise_sigma_pix(o.noise_sigma_e, o.noise_ngal, p.fov, p.npix, &noise_sigma_pix) != SLICER_OK ||
            slicer_noise_create(h, p.npix, o.noise_seed, nh.out()) != SLICER_OK)
            return fail(h, "slicer_amd: --shape-noise");
        for (size_t k = 0; k < o.smooth_arcmin.size(); k++) {
            noise_gain.push_back(0.0);
            if (slicer_smooth_noise_gain(o.smooth_kind == "map" ? SLICER_SMOOTH_MAP : SLICER_SMOOTH_GAUSS,
                                         o.smooth_sigma_pix(k, p.npix, p.fov), kSmoothTruncate, &noise_gain.back()) != SLICER_OK)
                return fail(h, "slicer_amd: --shape-noise");
        }
        for (double z : zs)  // (sources at one redshift share their stream, and with it their noise)
            noise_stream.push_back((uint32_t)std::count_if(zs.begin(), zs.end(), [z](double other) { return other < z; }));
    }
    if (o.starlet_scales > 0) {
        const int J = o.starlet_scales;
        starlet_gain.resize(J + 1);
        if (slicer_starlet_gains(J, &starlet_gain[1], &starlet_gain[0]) != SLICER_OK ||
            slicer_starlet_create(h, p.npix, J, sth.out()) != SLICER_OK)
            return fail(h, "slicer_amd: --starlet");
        for (int j = 1; j <= (o.shape_noise ? J : 1); j++) {
            vector<double> e = o.starlet_edges;
            if (o.shape_noise) {
                starlet_sigma.push_back(noise_sigma_pix * starlet_gain[j]);
                for (double &v : e)
                    v = v * starlet_sigma.back();
            }
            if (slicer_peaks_create(h, p.npix, (int)e.size(), e.data(), starlet_pkh.emplace_back().out()) != SLICER_OK ||
                slicer_l1norm_create(h, p.npix, (int)e.size(), e.data(), starlet_l1h.emplace_back().out()) != SLICER_OK)
                return fail(h, "slicer_amd: --starlet");
            starlet_scale_edges.push_back(e);
        }
    }
    if (o.scattering_J > 0 && slicer_scattering_create(h, p.npix, o.scattering_J, o.scattering_L, sch.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --scattering");
    if (!o.raytrace)
        return 0;
    if (slicer_kappa_create(h, p.npix, 1, lkh.out()) != SLICER_OK ||
        slicer_rays_create(h, p.npix, p.fov * M_PI / 180.0 / p.npix, rh.out()) != SLICER_OK)
        return fail(h, "slicer_amd: --raytrace");
    for (int k = 0; k < SLICER_RAYS_COUNT; k++)
        if (!rt_out.add(p.npix))
            return fail(h, "slicer_amd: --raytrace");
    rt_order.resize(zs.size());
    std::iota(rt_order.begin(), rt_order.end(), (size_t)0);
    std::stable_sort(rt_order.begin(), rt_order.end(), [&](size_t a, size_t b) { return zs[a] < zs[b]; });
    return observe_sources(0);  // the sources with no plane in front: from the start state
}

// --raytrace, plane i of the cone, whose mass map is d_map: its lens map L = strength (m - mean m) from the one-source
// kappa handle, the maps of L from the shear handle, one step of the rays, and the sources this plane is the last in
// front of.
int LensingOutputs::trace_plane(int i, const float *d_map)
{
    const char *who = "slicer_amd: --raytrace";
    const bool gradient = o.gradient();
    float *L = nullptr, *m[5] = {};
    const int spectral[5] = {SLICER_SHEAR_ALPHA1, SLICER_SHEAR_ALPHA2, -1, SLICER_SHEAR_GAMMA1, SLICER_SHEAR_GAMMA2};
    const int fd[5] = {SLICER_SHEAR_FD_ALPHA1, SLICER_SHEAR_FD_ALPHA2, SLICER_SHEAR_FD_KAPPA, SLICER_SHEAR_FD_GAMMA1,
                       SLICER_SHEAR_FD_GAMMA2};
    if (slicer_kappa_add(lkh, 1, &d_map, &plan.strength[i]) != SLICER_OK || slicer_kappa_finalize(lkh) != SLICER_OK ||
        slicer_kappa_device_map(lkh, 0, &L) != SLICER_OK || slicer_shear_run(shh, L) != SLICER_OK ||
        (gradient ? slicer_shear_fd(shh) : slicer_shear_deflection(shh)) != SLICER_OK)
        return fail(h, who);
    for (int k = 0; k < 5; k++) {
        const int which = gradient ? fd[k] : spectral[k];
        if (which < 0)
            m[k] = L;
        else if (slicer_shear_device_map(shh, which, &m[k]) != SLICER_OK)
            return fail(h, who);
    }
    if (slicer_rays_step(rh, plan.chil[i], m[0], m[1], m[2], m[3], m[4]) != SLICER_OK ||
        slicer_kappa_reset(lkh) != SLICER_OK)
        return fail(h, who);
    return observe_sources(i + 1);
}

// the sources, in ascending redshift, that have `done` planes in front of them: observed now and written
int LensingOutputs::observe_sources(int done)
{
    static const char *const token[SLICER_RAYS_COUNT] = {".rt_kappa_z", ".rt_gamma1_z", ".rt_gamma2_z",
                                                          ".rt_omega_z", ".rt_alpha1_z", ".rt_alpha2_z"};
    for (; rt_next < rt_order.size() && plan.in_front[rt_order[rt_next]] <= done; rt_next++) {
        const size_t s = rt_order[rt_next];
        if (slicer_rays_observe(rh, plan.chis[s], rt_out.maps.data()) != SLICER_OK)
            return fail(h, "slicer_amd: --raytrace");
        for (int k = 0; k < SLICER_RAYS_COUNT; k++)
            if (slicer_copy_to_host(h, map.data(), rt_out.maps[k], map.size() * sizeof(float)) != SLICER_OK ||
                !save("ray-traced", token[k], s))
                return fail(h, "slicer_amd: --raytrace");
    }
    return 0;
}

int LensingOutputs::add_pass(int i0, int i1, const vector<int> &todo)
{
    const size_t np2 = (size_t)p.npix * (size_t)p.npix;
    vector<const float *> maps;
    vector<double> c;
    vector<float> host;
    size_t n_up = 0;
    for (int i = i0; i < i1; i++) {
        const auto it = std::find(todo.begin(), todo.end(), i);
        float *d = nullptr;
        if (it != todo.end()) {
            if (slicer_plane_device_maps(h, (int)(it - todo.begin()), &d, nullptr) != SLICER_OK)
                return fail(h, "slicer_amd");
        } else {
            const string path = fileOutput(p, plane_label(lens.pll[i]));
            host.resize(np2);
            if (!fits_read_image(path, p.npix, host.data())) {
                cerr << "slicer_amd: --kappa: cannot read the plane back from " << path << endl;
                return 1;
            }
            if (upload.maps.size() <= n_up && !upload.add(p.npix))
                return fail(h, "slicer_amd");
            d = upload.maps[n_up++];
            // (stream-ordered after the previous batch's kernels, which may still read this buffer)
            if (slicer_copy_to_device(h, d, host.data(), np2 * sizeof(float)) != SLICER_OK)
                return fail(h, "slicer_amd");
        }
        maps.push_back(d);
        for (size_t s = 0; s < plan.zs.size(); s++)
            c.push_back(plan.coeff[s * lens.nplanes + i]);
    }
    if (slicer_kappa_add(kh, (int)maps.size(), maps.data(), c.data()) != SLICER_OK)
        return fail(h, "slicer_amd: --kappa");
    for (int i = i0; o.raytrace && i < i1; i++)
        if (const int rc = trace_plane(i, maps[i - i0]))
            return rc;
    return 0;
}

// `map` into <directory><simulation><token><z_s>_<npix>_<suffix>.fits with the keys of kslicer's genericHeader
bool LensingOutputs::save(const char *what, const string &token, size_t s, const vector<FitsKey> &more)
{
    char z[32];
    snprintf(z, sizeof z, "%.4f", plan.zs[s]);
    vector<FitsKey> keys = {{"ZSOURCE", false, 0, plan.zs[s], " "}, {"ANGLE", false, 0, p.fov, " "}};
    keys.insert(keys.end(), more.begin(), more.end());
    const string path = p.directory + p.simulation + token + z + "_" + p.snpix + "_" + p.suffix + ".fits";
    cout << "Saving the " << what << " map on: " << path << endl;
    if (fits_write_image(path, map.data(), p.npix, keys.data(), (int)keys.size()))
        return true;
    cerr << "It was not possible to create the map: " << path << endl;
    return false;
}

// Per source the kappa file, then its moments, then the histograms and the Minkowski functionals of its pyramid (which
// the moments of the same source left behind), then the shear files, then the smoothed maps with their moments,
// histograms and functionals, then the noisy maps with theirs; after the sources the tables, the Betti tables and then
// the scattering tables last.
int LensingOutputs::write()
{
    if (slicer_kappa_finalize(kh) != SLICER_OK)
        return fail(h, "slicer_amd: --kappa");
    for (size_t s = 0; s < plan.zs.size(); s++) {
        if (slicer_kappa_read(kh, (int)s, map.data()) != SLICER_OK || !save("convergence", ".kappa_z", s))
            return fail(h, "slicer_amd: --kappa");
        float *d_kappa = nullptr;
        if (slicer_kappa_device_map(kh, (int)s, &d_kappa) != SLICER_OK)
            return fail(h, "slicer_amd: --kappa");
        if (const int rc = map_statistics(s, d_kappa, KAPPA))
            return rc;
        if (const int rc = o.shear ? source_shear(s, d_kappa) : 0)
            return rc;
        if (const int rc = source_smooth(s, d_kappa))
            return rc;
        if (const int rc = nh ? source_noise(s, d_kappa) : 0)
            return rc;
        if (const int rc = sth ? source_starlet(s, d_kappa, false, ".", {}, "", "") : 0)
            return rc;
        if (const int rc = sch ? source_scattering(s, d_kappa, false, "", "") : 0)
            return rc;
    }
    if (const int rc = ph ? power_spectra() : 0)
        return rc;
    if (const int rc = pclh ? pseudo_spectra() : 0)
        return rc;
    if (const int rc = xih ? correlations() : 0)
        return rc;
    if (const int rc = bsh ? bispectra() : 0)
        return rc;
    // what stdout calls a statistic and its file token; the same of a kind of map, and whether the run has that kind
    static const char *const statistic[N_STATISTICS][2] = {
        {"moments", "moments_"}, {"histograms and peak counts", "peaks_"}, {"Minkowski functionals", "minkowski_"},
        {"Betti numbers", "betti_"}};
    static const char *const kind[N_KINDS][2] = {{"", "."},
                                                 {" of the smoothed maps", ".smooth_"},
                                                 {" of the noisy maps", ".noisy_"},
                                                 {" of the smoothed noisy maps", ".noisy_smooth_"}};
    const bool has_statistic[N_STATISTICS] = {mh != nullptr, pkh != nullptr, mkh != nullptr, bth != nullptr};
    const auto write_statistic = [&](int t, int k) {
        return write_table((string(statistic[t][0]) + kind[k][0]).c_str(), (string(kind[k][1]) + statistic[t][1]).c_str(),
                           tables[t][k]);
    };
    const bool has_kind[N_KINDS] = {true, !smh.empty(), nh != nullptr, nh != nullptr && !smh.empty()};
    // the moments and the histograms kind by kind, then the Minkowski tables: the order these files have always had
    for (const bool last : {false, true})
        for (int k = 0; k < N_KINDS; k++)
            for (int t = 0; t < N_STATISTICS; t++)
                if (t != BETTI && (t == MINKOWSKI) == last && has_statistic[t] && has_kind[k] && write_statistic(t, k))
                    return 1;
    static const char *const starlet_table[2][2] = {{"starlet histograms and peak counts", "starlet_peaks_"},
                                                    {"starlet l1-norms", "starlet_l1_"}};
    for (int noisy = 0; noisy < (sth ? (nh ? 2 : 1) : 0); noisy++)
        for (int t = 0; t < 2; t++)
            if (write_table((string(starlet_table[t][0]) + kind[noisy ? NOISY : KAPPA][0]).c_str(),
                            (string(kind[noisy ? NOISY : KAPPA][1]) + starlet_table[t][1]).c_str(), starlet_tables[t][noisy]))
                return 1;
    // the Betti tables after every file that a run without --betti writes
    for (int k = 0; k < N_KINDS; k++)
        if (has_statistic[BETTI] && has_kind[k] && write_statistic(BETTI, k))
            return 1;
    // ... and the scattering tables after those
    for (int noisy = 0; noisy < (sch ? (nh ? 2 : 1) : 0); noisy++)
        if (write_table((string("scattering coefficients") + kind[noisy ? NOISY : KAPPA][0]).c_str(),
                        (string(kind[noisy ? NOISY : KAPPA][1]) + "scattering_").c_str(), scattering_tables[noisy]))
            return 1;
    // ... and the catalogues last
    for (int k = 0; k < N_KINDS; k++)
        if (cth && has_kind[k] &&
            write_table((string("peak catalogues") + kind[k][0]).c_str(), (string(kind[k][1]) + "catalogue_").c_str(),
                        catalogue_tables[k]))
            return 1;
    return 0;
}

// The catalogue table: '#' lines (npix, angle, min_peak, capacity, `head`, the column names), then per map a '# map' line
// with its totals -- and a '# overflow' line where the capacity did not hold them -- and one row per stored record.
int LensingOutputs::source_catalogue(size_t s, const float *d_map, string &text, const string &head, const string &lead_names,
                                     const string &lead)
{
    const char *who = "slicer_amd: --catalogue";
    if (text.empty()) {
        add(text, "# npix %d\n# angle_deg %.17g\n# min_peak %.17g\n# capacity %lld\n", p.npix, p.fov, o.catalogue_min_peak,
            (long long)o.catalogue_capacity);
        text += head + "# z " + lead_names + "row col value dy dx off_row_deg off_col_deg flags\n";
    }
    int64_t n_peaks = 0, stored = 0, copied = 0;
    if (slicer_catalogue_run(cth, d_map, SLICER_CATALOGUE_PEAKS, o.catalogue_min_peak, INFINITY) != SLICER_OK ||
        slicer_catalogue_count(cth, &n_peaks, nullptr, &stored) != SLICER_OK)
        return fail(h, who);
    catalogue_records.resize((size_t)stored);
    if (slicer_catalogue_read(cth, catalogue_records.data(), stored, &copied) != SLICER_OK || copied != stored)
        return fail(h, who);
    string z;
    add(z, "%.17g ", plan.zs[s]);
    text += "# map " + z + lead;
    add(text, "n_peaks %lld stored %lld\n", (long long)n_peaks, (long long)stored);
    if (n_peaks > stored) {
        cerr << who << ": the map z " << lead_names << "= " << z << lead << "has " << n_peaks << " peaks, above the capacity: the first "
             << stored << " are listed" << endl;
        text += "# overflow " + z + lead;
        add(text, "%lld peaks are not listed\n", (long long)(n_peaks - stored));
    }
    const auto degrees = [&](int32_t pixel, double offset) { return ((((double)pixel + offset) + 0.5) / (double)p.npix - 0.5) * p.fov; };
    for (const slicer_catalogue_record &r : catalogue_records) {
        text += z + lead;
        add(text, "%d %d %.17g %.17g %.17g %.17g %.17g %u\n", (int)r.row, (int)r.col, (double)r.value, r.dy, r.dx,
            degrees(r.row, r.dy), degrees(r.col, r.dx), (unsigned)r.flags);
    }
    return 0;
}

// The scattering table: '#' lines (npix, angle, J, L, the filter constants, with --shape-noise its lines, the column
// names), then per source one row of order 0, J L rows of order 1 and J (J - 1) / 2 L^2 rows of order 2.
int LensingOutputs::source_scattering(size_t s, const float *d_map, bool noisy, const string &lead_names, const string &lead)
{
    const int J = o.scattering_J, L = o.scattering_L, JL = J * L;
    string &text = scattering_tables[noisy];
    if (text.empty()) {
        add(text, "# npix %d\n# angle_deg %.17g\n# J %d\n# L %d\n# sigma0 %.17g\n# xi0 %.17g\n# slant %.17g\n", p.npix, p.fov, J,
            L, 0.8, 3.0 * M_PI / 4.0, 4.0);
        text += (noisy ? noise_head() : "") + "# " + lead_names + "z order j1 l1 j2 l2 value power\n";
    }
    double s0[2];
    vector<double> s1(JL), p1(JL), s2((size_t)JL * JL);
    if (slicer_scattering_run(sch, d_map) != SLICER_OK ||
        slicer_scattering_read(sch, s0, s1.data(), p1.data(), s2.data()) != SLICER_OK)
        return fail(h, "slicer_amd: --scattering");
    const auto row = [&](int order, int j1, int l1, int j2, int l2, double value, double power) {
        text += lead;
        add(text, "%.17g %d %d %d %d %d %.17g %.17g\n", plan.zs[s], order, j1, l1, j2, l2, value, power);
    };
    row(0, -1, -1, -1, -1, s0[0], s0[1]);
    for (int a = 0; a < JL; a++)
        row(1, a / L, a % L, -1, -1, s1[a], p1[a]);
    for (int a = 0; a < JL; a++)
        for (int b = (a / L + 1) * L; b < JL; b++)
            row(2, a / L, a % L, b / L, b % L, s2[(size_t)a * JL + b], NAN);
    return 0;
}

// --starlet: the J + 1 maps of the map at d_map, and per scale j = 1 ... J the rows of the two tables.  Both tables: '#'
// lines (npix, angle, scales, the edges as given, the gains of w_1 ... w_J, with --shape-noise its lines and sigma_scale,
// the column names), then per (source, scale) one row per bin: -1 (below the first edge), 0 ... B-1, B (above the last),
// B+1 (NaN pixels); edge_lo and edge_hi are the scale's own edges.
int LensingOutputs::source_starlet(size_t s, const float *d_map, bool noisy, const string &prefix, const vector<FitsKey> &keys,
                                   const string &lead_names, const string &lead)
{
    const char *who = "slicer_amd: --starlet";
    const int J = o.starlet_scales, B = (int)o.starlet_edges.size() - 1;
    string &pk = starlet_tables[0][noisy], &l1 = starlet_tables[1][noisy];
    if (pk.empty()) {
        string head;
        add(head, "# npix %d\n# angle_deg %.17g\n# scales %d\n# edges", p.npix, p.fov, J);
        for (double v : o.starlet_edges)
            add(head, " %.17g", v);
        add(head, "\n# gain");
        for (int j = 1; j <= J; j++)
            add(head, " %.17g", starlet_gain[j]);
        head += "\n";
        if (nh) {
            head += noise_head() + "# sigma_scale";
            for (double v : starlet_sigma)
                add(head, " %.17g", v);
            head += "\n";
        }
        pk = head + "# " + lead_names + "z scale bin edge_lo edge_hi n_pixels n_peaks n_minima\n";
        l1 = head + "# " + lead_names + "z scale bin edge_lo edge_hi count l1\n";
    }
    if (slicer_starlet_run(sth, d_map) != SLICER_OK)
        return fail(h, who);
    vector<int64_t> c(3 * B + 7), n(B + 3);  // peaks: pdf, peaks, minima [B], below, above [3], nan; l1: counts [B], below, above, nan
    vector<double> sum(B + 2);               // ... the sums [B], below, above
    for (int j = 0; j <= J; j++) {
        float *d_w = nullptr;
        if (slicer_starlet_read(sth, j, map.data()) != SLICER_OK || slicer_starlet_device_map(sth, j, &d_w) != SLICER_OK)
            return fail(h, who);
        char gain[32];
        snprintf(gain, sizeof gain, "%.17g", starlet_gain[j]);
        vector<FitsKey> more = keys;
        more.push_back({"SCALE", true, j, 0.0, " "});
        more.push_back({"GAIN", false, 0, starlet_gain[j], " ", gain});
        if (!save(noisy ? "noisy starlet" : "starlet", prefix + "starlet" + std::to_string(j) + "_kappa_z", s, more))
            return fail(h, who);
        if (j == 0)
            continue;
        const size_t set = std::min<size_t>(j - 1, starlet_scale_edges.size() - 1);
        const vector<double> &e = starlet_scale_edges[set];
        if (slicer_peaks_run(starlet_pkh[set], d_w) != SLICER_OK ||
            slicer_peaks_read(starlet_pkh[set], &c[0], &c[B], &c[2 * B], &c[3 * B], &c[3 * B + 3], &c[3 * B + 6]) != SLICER_OK ||
            slicer_l1norm_run(starlet_l1h[set], d_w) != SLICER_OK ||
            slicer_l1norm_read(starlet_l1h[set], &n[0], &sum[0], &n[B], &n[B + 1], &n[B + 2], &sum[B], &sum[B + 1]) != SLICER_OK)
            return fail(h, who);
        const auto row = [&](int bin, double lo, double hi, int64_t n_pixels, int64_t n_peaks, int64_t n_minima, int64_t count,
                             double total) {
            pk += lead;
            add(pk, "%.17g %d %d %.17g %.17g %lld %lld %lld\n", plan.zs[s], j, bin, lo, hi, (long long)n_pixels,
                (long long)n_peaks, (long long)n_minima);
            l1 += lead;
            add(l1, "%.17g %d %d %.17g %.17g %lld %.17g\n", plan.zs[s], j, bin, lo, hi, (long long)count, total);
        };
        row(-1, -INFINITY, e[0], c[3 * B], c[3 * B + 1], c[3 * B + 2], n[B], sum[B]);
        for (int b = 0; b < B; b++)
            row(b, e[b], e[b + 1], c[b], c[B + b], c[2 * B + b], n[b], sum[b]);
        row(B, e[B], INFINITY, c[3 * B + 3], c[3 * B + 4], c[3 * B + 5], n[B + 1], sum[B + 1]);
        row(B + 1, NAN, NAN, c[3 * B + 6], 0, 0, n[B + 2], 0.0);
    }
    return 0;
}

// the '#' lines of --smooth in the tables of the smoothed maps
string LensingOutputs::smooth_head() const
{
    string head;
    add(head, "# smooth %s\n# scales_arcmin", o.smooth_kind.c_str());
    for (double a : o.smooth_arcmin)
        add(head, " %.17g", a);
    add(head, "\n# sigma_pix");
    for (size_t k = 0; k < smh.size(); k++)
        add(head, " %.17g", o.smooth_sigma_pix(k, p.npix, p.fov));
    add(head, "\n# radius");
    for (int32_t r : smooth_radius)
        add(head, " %d", (int)r);
    add(head, "\n");
    return head;
}

// the '#' lines of --shape-noise in the tables of the noisy maps
string LensingOutputs::noise_head() const
{
    string head;
    add(head, "# sigma_e %.17g\n# ngal_arcmin2 %.17g\n# noise_sigma_pix %.17g\n# seed %llu\n# nreal %d\n", o.noise_sigma_e,
        o.noise_ngal, noise_sigma_pix, (unsigned long long)o.noise_seed, o.noise_nreal);
    return head;
}

// --shape-noise: per realisation r the noisy kappa map of source s, .noisy<r>_kappa_z, its rows of the two tables, and
// with --smooth every scale of the noisy map, .noisy<r>_<kind><k>_kappa_z, with the rows of those
int LensingOutputs::source_noise(size_t s, const float *d_kappa)
{
    const char *who = "slicer_amd: --shape-noise";
    const string head = noise_head();
    string smoothed_head = smh.empty() ? "" : smooth_head() + head + "# noise_sigma";
    for (double g : noise_gain)
        add(smoothed_head, " %.17g", noise_sigma_pix * g);
    smoothed_head += "\n";
    for (int r = 0; r < o.noise_nreal; r++) {
        float *d_noisy = nullptr;
        if (slicer_noise_run(nh, d_kappa, noise_sigma_pix, noise_stream[s], (uint32_t)r) != SLICER_OK ||
            slicer_noise_read(nh, map.data()) != SLICER_OK || slicer_noise_device_map(nh, &d_noisy) != SLICER_OK)
            return fail(h, who);
        const vector<FitsKey> keys = {{"SIGMAE", false, 0, o.noise_sigma_e, " "},
                                      {"NGAL", false, 0, o.noise_ngal, " "},
                                      {"SIGMAPIX", false, 0, noise_sigma_pix, " "},
                                      {"SEED", true, (long)o.noise_seed, 0.0, " "},
                                      {"REALIS", true, r, 0.0, " "}};
        const string real = std::to_string(r);
        if (!save("noisy convergence", ".noisy" + real + "_kappa_z", s, keys))
            return fail(h, who);
        if (const int rc = map_statistics(s, d_noisy, NOISY, head, "real ", real + " "))
            return rc;
        for (size_t k = 0; k < smh.size(); k++) {
            float *d_smooth = nullptr;
            if (slicer_smooth_run(smh[k], d_noisy) != SLICER_OK || slicer_smooth_read(smh[k], map.data()) != SLICER_OK ||
                slicer_smooth_device_map(smh[k], &d_smooth) != SLICER_OK)
                return fail(h, who);
            vector<FitsKey> more = keys;
            more.push_back({"SCALE", false, 0, o.smooth_arcmin[k], " "});
            more.push_back({"RADIUS", true, smooth_radius[k], 0.0, " "});
            more.push_back({"NOISESIG", false, 0, noise_sigma_pix * noise_gain[k], " "});
            const string lead = real + " " + std::to_string(k) + " ";
            if (!save("smoothed noisy convergence", ".noisy" + real + "_" + o.smooth_kind + std::to_string(k) + "_kappa_z", s,
                      more))
                return fail(h, who);
            if (const int rc = map_statistics(s, d_smooth, NOISY_SMOOTH, smoothed_head, "real scale ", lead))
                return rc;
        }
        if (const int rc = sth ? source_starlet(s, d_noisy, true, ".noisy" + real + "_", keys, "real ", real + " ") : 0)
            return rc;
        if (const int rc = sch ? source_scattering(s, d_noisy, true, "real ", real + " ") : 0)
            return rc;
    }
    return 0;
}

// --smooth: per scale k the smoothed kappa map of source s, .<kind><k>_kappa_z, and its rows of the two tables
int LensingOutputs::source_smooth(size_t s, const float *d_kappa)
{
    if (smh.empty())
        return 0;
    const string head = smooth_head();  // of both tables
    for (size_t k = 0; k < smh.size(); k++) {
        float *d_smooth = nullptr;
        if (slicer_smooth_run(smh[k], d_kappa) != SLICER_OK || slicer_smooth_read(smh[k], map.data()) != SLICER_OK ||
            slicer_smooth_device_map(smh[k], &d_smooth) != SLICER_OK)
            return fail(h, "slicer_amd: --smooth");
        const vector<FitsKey> keys = {{"SCALE", false, 0, o.smooth_arcmin[k], " "}, {"RADIUS", true, smooth_radius[k], 0.0, " "}};
        if (!save("smoothed convergence", "." + o.smooth_kind + std::to_string(k) + "_kappa_z", s, keys))
            return fail(h, "slicer_amd: --smooth");
        const string lead = std::to_string(k) + " ";
        if (const int rc = map_statistics(s, d_smooth, SMOOTH, head, "scale ", lead))
            return rc;
    }
    return 0;
}

int LensingOutputs::map_statistics(size_t s, float *d_map, MapKind kind, const string &head, const string &lead_names,
                                   const string &lead)
{
    if (const int rc = mh ? source_moments(s, d_map, tables[MOMENTS][kind], head, lead_names, lead) : 0)
        return rc;
    if (const int rc = pkh ? source_peaks(s, d_map, tables[PEAKS][kind], head, lead_names, lead) : 0)
        return rc;
    if (const int rc = mkh ? source_minkowski(s, d_map, tables[MINKOWSKI][kind], head, lead_names, lead) : 0)
        return rc;
    if (const int rc = bth ? source_betti(s, d_map, tables[BETTI][kind], head, lead_names, lead) : 0)
        return rc;
    return cth ? source_catalogue(s, d_map, catalogue_tables[kind], head, lead_names, lead) : 0;
}

void LensingOutputs::counts_head(string &text, const char *name, const vector<double> &values, const string &head,
                                 const string &columns) const
{
    if (!text.empty())
        return;
    add(text, "# npix %d\n# angle_deg %.17g\n# levels %d\n# %s", p.npix, p.fov, mh ? o.moments_levels : 0, name);
    for (double v : values)
        add(text, " %.17g", v);
    text += "\n" + head + "# " + columns;
}

template <class Rows>
int LensingOutputs::pyramid_levels(const char *who, float *d_map, Rows rows)
{
    for (int l = 0; l <= (mh ? o.moments_levels : 0); l++) {
        float *d_level = d_map;
        if (l > 0 && slicer_moments_device_map(mh, l, &d_level) != SLICER_OK)
            return fail(h, who);
        if (const int rc = rows(l, d_level))
            return rc;
    }
    return 0;
}

// The moments table: '#' lines (npix, angle, levels, column names), then per (source, level) z level npix mean S2 ... S8
// (%.17g): the raw sums about the level's own mean.  The tables of the smoothed and the noisy maps: `head` before the
// column names, `lead_names` in front of them and `lead` in front of every row.
int LensingOutputs::source_moments(size_t s, const float *d_map, string &text, const string &head, const string &lead_names,
                                   const string &lead)
{
    const int nlev = o.moments_levels + 1;
    vector<int32_t> npix(nlev);
    vector<double> mean(nlev), sums(nlev * SLICER_MOMENTS_ORDERS);
    if (slicer_moments_run(mh, d_map, nullptr) != SLICER_OK ||
        slicer_moments_read(mh, npix.data(), mean.data(), nullptr, sums.data()) != SLICER_OK)
        return fail(h, "slicer_amd: --moments");
    if (text.empty()) {
        add(text, "# npix %d\n# angle_deg %.17g\n# levels %d\n", p.npix, p.fov, o.moments_levels);
        text += head + "# " + lead_names + "z level npix mean";
        for (int k = 2; k < 2 + SLICER_MOMENTS_ORDERS; k++)
            add(text, " S%d", k);
        add(text, "\n");
    }
    for (int l = 0; l < nlev; l++) {
        text += lead;
        add(text, "%.17g %d %d %.17g", plan.zs[s], l, (int)npix[l], mean[l]);
        for (int k = 0; k < SLICER_MOMENTS_ORDERS; k++)
            add(text, " %.17g", sums[l * SLICER_MOMENTS_ORDERS + k]);
        add(text, "\n");
    }
    return 0;
}

// The histogram table: '#' lines (npix, angle, levels, the edges, column names), then per (source, level) one row per
// bin: -1 (below the first edge), 0 ... B-1, B (above the last), B+1 (NaN pixels).  The levels are those of the pyramid
// that the moments of this source left behind (level 0 alone without --moments).
int LensingOutputs::source_peaks(size_t s, float *d_map, string &text, const string &head, const string &lead_names,
                                 const string &lead)
{
    const vector<double> &e = o.peaks_edges;
    const int B = (int)e.size() - 1;
    vector<int64_t> c(3 * B + 7);  // pdf, peaks, minima [B]; below, above [3]; nan
    const int64_t *below = &c[3 * B], *above = below + 3;
    counts_head(text, "edges", e, head, lead_names + "z level npix bin lo hi n_pixels n_peaks n_minima\n");
    return pyramid_levels("slicer_amd: --peaks", d_map, [&](int l, float *d_level) {
        if (slicer_peaks_run_npix(pkh, d_level, p.npix >> l) != SLICER_OK ||
            slicer_peaks_read(pkh, &c[0], &c[B], &c[2 * B], &c[3 * B], &c[3 * B + 3], &c[3 * B + 6]) != SLICER_OK)
            return fail(h, "slicer_amd: --peaks");
        const auto row = [&](int bin, double lo, double hi, int64_t n_pixels, int64_t n_peaks, int64_t n_minima) {
            text += lead;
            add(text, "%.17g %d %d %d %.17g %.17g %lld %lld %lld\n", plan.zs[s], l, p.npix >> l, bin, lo, hi,
                (long long)n_pixels, (long long)n_peaks, (long long)n_minima);
        };
        row(-1, -INFINITY, e[0], below[0], below[1], below[2]);
        for (int b = 0; b < B; b++)
            row(b, e[b], e[b + 1], c[b], c[B + b], c[2 * B + b]);
        row(B, e[B], INFINITY, above[0], above[1], above[2]);
        row(B + 1, NAN, NAN, c[3 * B + 6], 0, 0);
        return 0;
    });
}

// The Minkowski table: '#' lines (npix, angle, levels, the thresholds, column names), then per (source, level) one row
// per threshold j: the exact counts of slicer_minkowski_read and euler = n_vertices - n_edges + n_faces; n_nan is the
// level's, repeated in every row.  The levels are those of source_peaks.
int LensingOutputs::source_minkowski(size_t s, float *d_map, string &text, const string &head, const string &lead_names,
                                     const string &lead)
{
    const vector<double> &t = o.minkowski_thresholds;
    const int T = (int)t.size();
    vector<int64_t> c(5 * T);  // faces, edges, vertices, boundary, border [T]
    int64_t n_nan = 0;
    counts_head(text, "thresholds", t, head,
                lead_names + "z level npix j threshold n_faces n_edges n_vertices n_boundary n_border euler n_nan\n");
    return pyramid_levels("slicer_amd: --minkowski", d_map, [&](int l, float *d_level) {
        if (slicer_minkowski_run_npix(mkh, d_level, p.npix >> l) != SLICER_OK ||
            slicer_minkowski_read(mkh, &c[0], &c[T], &c[2 * T], &c[3 * T], &c[4 * T], &n_nan) != SLICER_OK)
            return fail(h, "slicer_amd: --minkowski");
        for (int j = 0; j < T; j++) {
            text += lead;
            add(text, "%.17g %d %d %d %.17g %lld %lld %lld %lld %lld %lld %lld\n", plan.zs[s], l, p.npix >> l, j, t[j],
                (long long)c[j], (long long)c[T + j], (long long)c[2 * T + j], (long long)c[3 * T + j],
                (long long)c[4 * T + j], (long long)(c[2 * T + j] - c[T + j] + c[j]), (long long)n_nan);
        }
        return 0;
    });
}

// The Betti table: '#' lines (npix, angle, levels, the thresholds, column names), then per (source, level) one row per
// threshold j: the exact counts of slicer_betti_read; n_nan is the level's, repeated in every row.  The levels are those
// of source_peaks.
int LensingOutputs::source_betti(size_t s, float *d_map, string &text, const string &head, const string &lead_names,
                                 const string &lead)
{
    const vector<double> &t = o.betti_thresholds;
    const int T = (int)t.size();
    vector<int64_t> c(3 * T);  // components, holes, faces [T]
    int64_t n_nan = 0;
    counts_head(text, "thresholds", t, head, lead_names + "z level npix j threshold n_components n_holes n_faces n_nan\n");
    return pyramid_levels("slicer_amd: --betti", d_map, [&](int l, float *d_level) {
        if (slicer_betti_run_npix(bth, d_level, p.npix >> l) != SLICER_OK ||
            slicer_betti_read(bth, &c[0], &c[T], &c[2 * T], &n_nan) != SLICER_OK)
            return fail(h, "slicer_amd: --betti");
        for (int j = 0; j < T; j++) {
            text += lead;
            add(text, "%.17g %d %d %d %.17g %lld %lld %lld %lld\n", plan.zs[s], l, p.npix >> l, j, t[j], (long long)c[j],
                (long long)c[T + j], (long long)c[2 * T + j], (long long)n_nan);
        }
        return 0;
    });
}

// smr.smr(kappa file): next to the kappa file, the same name with the .kappa_z token replaced, the same header
int LensingOutputs::source_shear(size_t s, const float *d_kappa)
{
    static const char *const token[6] = {".gamma1_z", ".gamma2_z", ".gamma_z", ".phi_z", ".alpha1_z", ".alpha2_z"};
    const int spectral[6] = {SLICER_SHEAR_GAMMA1, SLICER_SHEAR_GAMMA2, SLICER_SHEAR_GAMMA,
                             SLICER_SHEAR_PHI,    SLICER_SHEAR_ALPHA1, SLICER_SHEAR_ALPHA2};
    const int fd[6] = {SLICER_SHEAR_FD_GAMMA1, SLICER_SHEAR_FD_GAMMA2, SLICER_SHEAR_FD_GAMMA,
                       SLICER_SHEAR_PHI,       SLICER_SHEAR_FD_ALPHA1, SLICER_SHEAR_FD_ALPHA2};
    const bool g = o.gradient();
    if (slicer_shear_run(shh, d_kappa) != SLICER_OK)
        return fail(h, "slicer_amd: --kappa");
    if ((g && slicer_shear_fd(shh) != SLICER_OK) || (o.deflection && !g && slicer_shear_deflection(shh) != SLICER_OK))
        return fail(h, "slicer_amd: --shear");
    for (int k = 0; k < (o.deflection ? 6 : 4); k++) {
        if (slicer_shear_read(shh, g ? fd[k] : spectral[k], map.data()) != SLICER_OK ||
            !save(k < 4 ? "shear" : "deflection", token[k], s))
            return fail(h, "slicer_amd: --kappa");
        if (pcl2h && k < 2 &&  // the gamma just written, kept on the device for --pcl-shear
            slicer_copy_to_device(h, pcl2_gamma.maps[2 * s + k], map.data(), map.size() * sizeof(float)) != SLICER_OK)
            return fail(h, "slicer_amd: --pcl-shear");
    }
    if (xipmh) {  // xi+ and xi- of the gammas just written
        const int B = (int)o.xi_edges.size() - 1;
        float *g12[2] = {nullptr, nullptr};
        xipm_rows.resize((s + 1) * 2 * (size_t)B);
        double *row = &xipm_rows[s * 2 * (size_t)B];
        if (slicer_shear_device_map(shh, g ? fd[0] : spectral[0], &g12[0]) != SLICER_OK ||
            slicer_shear_device_map(shh, g ? fd[1] : spectral[1], &g12[1]) != SLICER_OK ||
            slicer_xi_run(xipmh, g12) != SLICER_OK ||
            slicer_xi_read(xipmh, row, row + B, nullptr, nullptr, nullptr) != SLICER_OK)
            return fail(h, "slicer_amd: --xi");
    }
    return 0;
}

// The spectra table: '#' lines (npix, angle, source redshifts, column names), then per bin ell_lo ell_hi ell_mean n_modes
// and C of every pair (%.17g; nan for an empty bin)
int LensingOutputs::power_spectra()
{
    const int S = (int)plan.zs.size(), B = o.n_power_edges(p.npix) - 1;
    const bool cross = o.power == "cross";
    const size_t n_pairs = cross ? (size_t)S * (S + 1) / 2 : S;
    vector<float *> maps(S);
    for (int s = 0; s < S; s++)
        if (slicer_kappa_device_map(kh, s, &maps[s]) != SLICER_OK)
            return fail(h, "slicer_amd: --power");
    vector<double> c(n_pairs * B), ell(B);
    vector<int64_t> counts(B);
    if (slicer_power_run(ph, maps.data()) != SLICER_OK ||
        slicer_power_read(ph, c.data(), ell.data(), counts.data()) != SLICER_OK)
        return fail(h, "slicer_amd: --power");
    const double ell_f = 2.0 * M_PI / (p.fov * M_PI / 180.0);
    string cl;
    add(cl, "# npix %d\n# angle_deg %.17g\n# zs", p.npix, p.fov);
    for (double z : plan.zs)
        add(cl, " %.17g", z);
    add(cl, "\n# ell_lo ell_hi ell_mean n_modes");
    for (int s = 0; s < S; s++)
        for (int t = s; t < (cross ? S : s + 1); t++)
            add(cl, " C_%d_%d", s, t);
    add(cl, "\n");
    for (int b = 0; b < B; b++) {
        const double lo = o.power_edges.empty() ? (double)b : o.power_edges[b];
        const double hi = o.power_edges.empty() ? (double)(b + 1) : o.power_edges[b + 1];
        add(cl, "%.17g %.17g %.17g %lld", lo * ell_f, hi * ell_f, ell[b], (long long)counts[b]);
        for (size_t q = 0; q < n_pairs; q++)
            add(cl, " %.17g", c[q * B + b]);
        add(cl, "\n");
    }
    return write_table("power spectra", ".cl_", cl);
}

// --pcl.  The pseudo-spectra table: the '#' lines of the spectra table with mean_w, mean_w2, taper_arcmin, taper_pix (0
// without --pcl-taper) and mask (the file as given, "none" without --pcl-mask) before the column names, then per bin
// ell_lo ell_hi ell_mean n_modes and per pair the decoupled C and the coupled Ct (%.17g; nan for an empty bin).  The matrix
// table: '#' lines (npix, the bin edges in multipoles), then row b of M per line (%.17g).
int LensingOutputs::pseudo_spectra()
{
    const char *who = "slicer_amd: --pcl";
    const int S = (int)plan.zs.size(), B = (int)o.pcl_edges.size() - 1;
    const bool cross = o.pcl == "cross";
    const size_t n_pairs = cross ? (size_t)S * (S + 1) / 2 : S;
    const double taper_pix = o.pcl_taper_given ? o.pcl_taper_pix(p.npix, p.fov) : 0.0;
    DeviceMaps mask(h);
    if (!o.pcl_mask.empty()) {
        vector<float> w((size_t)p.npix * (size_t)p.npix);
        const string why = fits_read_mask(o.pcl_mask, p.npix, w.data());
        if (!why.empty()) {
            cerr << who << "-mask: " << why << endl;
            return 1;
        }
        if (!mask.add(p.npix) || slicer_copy_to_device(h, mask.maps[0], w.data(), w.size() * sizeof(float)) != SLICER_OK)
            return fail(h, who);
    }
    // (slicer_pcl_set_mask waits for the stream: the host copy of the mask is no longer read when it returns)
    if (slicer_pcl_set_mask(pclh, mask.maps.empty() ? nullptr : mask.maps[0], taper_pix) != SLICER_OK)
        return fail(h, who);
    vector<float *> maps(S);
    for (int s = 0; s < S; s++)
        if (slicer_kappa_device_map(kh, s, &maps[s]) != SLICER_OK)
            return fail(h, who);
    vector<double> c(n_pairs * B), ct(n_pairs * B), ell(B), M((size_t)B * B);
    vector<int64_t> counts(B);
    double mean_w = 0.0, mean_w2 = 0.0;
    if (slicer_pcl_run(pclh, maps.data()) != SLICER_OK ||
        slicer_pcl_read(pclh, c.data(), ct.data(), ell.data(), counts.data()) != SLICER_OK ||
        slicer_pcl_coupling(pclh, M.data(), &mean_w, &mean_w2) != SLICER_OK)
        return fail(h, who);
    const double ell_f = 2.0 * M_PI / (p.fov * M_PI / 180.0);
    string cl;
    add(cl, "# npix %d\n# angle_deg %.17g\n# zs", p.npix, p.fov);
    for (double z : plan.zs)
        add(cl, " %.17g", z);
    add(cl, "\n# mean_w %.17g\n# mean_w2 %.17g\n# taper_arcmin %.17g\n# taper_pix %.17g\n# mask ", mean_w, mean_w2,
        o.pcl_taper_arcmin, taper_pix);
    cl += o.pcl_mask.empty() ? "none" : o.pcl_mask;
    add(cl, "\n# ell_lo ell_hi ell_mean n_modes");
    const string head = cl;  // the '#' lines up to the first column names
    for (int s = 0; s < S; s++)
        for (int t = s; t < (cross ? S : s + 1); t++)
            add(cl, " C_%d_%d Ct_%d_%d", s, t, s, t);
    add(cl, "\n");
    for (int b = 0; b < B; b++) {
        add(cl, "%.17g %.17g %.17g %lld", o.pcl_edges[b] * ell_f, o.pcl_edges[b + 1] * ell_f, ell[b], (long long)counts[b]);
        for (size_t q = 0; q < n_pairs; q++)
            add(cl, " %.17g %.17g", c[q * B + b], ct[q * B + b]);
        add(cl, "\n");
    }
    if (const int rc = write_table("pseudo-spectra", ".pcl_", cl))
        return rc;
    string m;
    add(m, "# npix %d\n# ell_edges", p.npix);
    for (double r : o.pcl_edges)
        add(m, " %.17g", r * ell_f);
    add(m, "\n");
    for (int b = 0; b < B; b++)
        for (int k = 0; k < B; k++)
            add(m, k + 1 < B ? "%.17g " : "%.17g\n", M[(size_t)b * B + k]);
    if (const int rc = write_table("mode-coupling matrix", ".pclm_", m))
        return rc;
    return pcl2h ? shear_pseudo_spectra(mask.maps.empty() ? nullptr : mask.maps[0], taper_pix, head) : 0;
}

// --pcl-shear, after --pcl's own tables, with its mask.  The E/B table: `head` (the '#' lines of the .pcl_ table and its
// bin columns' names), the names of the columns described at the top of this file, then per bin ell_lo ell_hi ell_mean
// n_modes and per column pair the decoupled C and the coupled Ct (%.17g; nan for an empty bin).  The matrix table: '#'
// lines (npix, the bin edges in multipoles), then under '# M0', '# M2', '# X2', '# M4', '# X4' the rows of each (%.17g).
int LensingOutputs::shear_pseudo_spectra(const float *d_mask, double taper_pix, const string &head)
{
    const char *who = "slicer_amd: --pcl-shear";
    const int S = (int)plan.zs.size(), B = (int)o.pcl_edges.size() - 1;
    const bool cross = o.pcl == "cross";
    const size_t n_rows = cross ? (size_t)(3 * S) * (3 * S + 1) / 2 : (size_t)6 * S;
    if (slicer_pcl2_set_mask(pcl2h, d_mask, taper_pix) != SLICER_OK)
        return fail(h, who);
    vector<float *> maps(3 * (size_t)S);
    for (int s = 0; s < S; s++) {
        maps[3 * s] = pcl2_gamma.maps[2 * s];
        maps[3 * s + 1] = pcl2_gamma.maps[2 * s + 1];
        if (slicer_kappa_device_map(kh, s, &maps[3 * s + 2]) != SLICER_OK)
            return fail(h, who);
    }
    vector<double> c(n_rows * B), ct(n_rows * B), ell(B), M[5];
    vector<int64_t> counts(B);
    for (auto &m : M)
        m.resize((size_t)B * B);
    if (slicer_pcl2_run(pcl2h, maps.data()) != SLICER_OK ||
        slicer_pcl2_read(pcl2h, c.data(), ct.data(), ell.data(), counts.data()) != SLICER_OK ||
        slicer_pcl2_coupling(pcl2h, M[0].data(), M[1].data(), M[2].data(), M[3].data(), M[4].data(), nullptr, nullptr) !=
            SLICER_OK)
        return fail(h, who);
    // the table row of (component a of source s, component b of source t), a, b = 0, 1, 2 for E, B, kappa: the pair
    // order of slicer_pcl2_create
    const auto pair_of = [](int i, int j, int n) {
        if (i > j)
            std::swap(i, j);
        return i * n - i * (i - 1) / 2 + (j - i);
    };
    const auto row = [&](int s, int a, int t, int b) {
        return cross ? (size_t)pair_of(3 * s + a, 3 * t + b, 3 * S) : (size_t)6 * s + pair_of(a, b, 3);
    };
    struct Column {
        string name;
        size_t row;
    };
    vector<Column> cols;
    static const char letter[3] = {'E', 'B', 'k'};
    const auto column = [&](int s, int a, int t, int b) {
        cols.push_back({string(1, letter[a]) + letter[b] + "_" + std::to_string(s) + "_" + std::to_string(t), row(s, a, t, b)});
    };
    for (int s = 0; s < S; s++)
        for (int t = s; t < (cross ? S : s + 1); t++) {
            column(s, 0, t, 0);
            column(s, 0, t, 1);
            if (s < t)
                column(s, 1, t, 0);
            column(s, 1, t, 1);
            column(s, 2, t, 0);
            column(s, 2, t, 1);
            if (s < t) {
                column(t, 2, s, 0);
                column(t, 2, s, 1);
            }
        }
    const double ell_f = 2.0 * M_PI / (p.fov * M_PI / 180.0);
    string cl = head;
    for (const Column &q : cols)
        cl += " C_" + q.name + " Ct_" + q.name;
    cl += "\n";
    for (int b = 0; b < B; b++) {
        add(cl, "%.17g %.17g %.17g %lld", o.pcl_edges[b] * ell_f, o.pcl_edges[b + 1] * ell_f, ell[b], (long long)counts[b]);
        for (const Column &q : cols)
            add(cl, " %.17g %.17g", c[q.row * B + b], ct[q.row * B + b]);
        add(cl, "\n");
    }
    if (const int rc = write_table("E/B pseudo-spectra", ".pcleb_", cl))
        return rc;
    static const char *const name[5] = {"M0", "M2", "X2", "M4", "X4"};
    string m;
    add(m, "# npix %d\n# ell_edges", p.npix);
    for (double r : o.pcl_edges)
        add(m, " %.17g", r * ell_f);
    add(m, "\n");
    for (int k = 0; k < 5; k++) {
        add(m, "# %s\n", name[k]);
        for (int b = 0; b < B; b++)
            for (int j = 0; j < B; j++)
                add(m, j + 1 < B ? "%.17g " : "%.17g\n", M[k][(size_t)b * B + j]);
    }
    return write_table("spin-2 coupling matrices", ".pclebm_", m);
}

// --xi.  Both tables: '#' lines (npix, angle, source redshifts, mask: the file as given or "none", padded: P, the column
// names), then per bin r_lo r_hi r_mean in arcminutes, the xi columns, W_b and N_b (%.17g; nan for an empty bin).  The
// .xi_ table has xi_s_t of every pair of kappa maps, the .xipm_ table (with --shear) xip_s xim_s of every source.
int LensingOutputs::correlations()
{
    const char *who = "slicer_amd: --xi";
    const int S = (int)plan.zs.size(), B = (int)o.xi_edges.size() - 1;
    const bool cross = o.xi == "cross";
    const size_t n_pairs = cross ? (size_t)S * (S + 1) / 2 : S;
    const vector<double> e = o.xi_edges_pix(p.npix, p.fov);
    int32_t P = 0;
    vector<float *> maps(S);
    for (int s = 0; s < S; s++)
        if (slicer_kappa_device_map(kh, s, &maps[s]) != SLICER_OK)
            return fail(h, who);
    vector<double> c(n_pairs * B), r(B), W(B);
    vector<int64_t> counts(B);
    if (slicer_xi_bins(p.npix, B + 1, e.data(), nullptr, nullptr, &P) != SLICER_OK)
        return fail(nullptr, who);
    if (slicer_xi_run(xih, maps.data()) != SLICER_OK ||
        slicer_xi_read(xih, c.data(), nullptr, r.data(), W.data(), counts.data()) != SLICER_OK)
        return fail(h, who);
    const double arcmin = 60.0 * p.fov / p.npix;  // of one pixel
    string head;
    add(head, "# npix %d\n# angle_deg %.17g\n# zs", p.npix, p.fov);
    for (double z : plan.zs)
        add(head, " %.17g", z);
    head += "\n# mask " + (o.xi_mask.empty() ? string("none") : o.xi_mask);
    add(head, "\n# padded %d\n# r_lo r_hi r_mean", (int)P);
    for (const bool pm : {false, true}) {
        if (pm && !xipmh)
            break;
        string t = head;
        for (int s = 0; s < S; s++)
            if (pm)
                add(t, " xip_%d xim_%d", s, s);
            else
                for (int u = s; u < (cross ? S : s + 1); u++)
                    add(t, " xi_%d_%d", s, u);
        t += " weight n_pairs\n";
        for (int b = 0; b < B; b++) {
            add(t, "%.17g %.17g %.17g", o.xi_edges[b], o.xi_edges[b + 1], r[b] * arcmin);
            if (pm)
                for (int s = 0; s < S; s++)
                    add(t, " %.17g %.17g", xipm_rows[((size_t)s * 2) * B + b], xipm_rows[((size_t)s * 2 + 1) * B + b]);
            else
                for (size_t q = 0; q < n_pairs; q++)
                    add(t, " %.17g", c[q * B + b]);
            add(t, " %.17g %lld\n", W[b], (long long)counts[b]);
        }
        if (const int rc = pm ? write_table("shear correlation functions", ".xipm_", t)
                              : write_table("correlation functions", ".xi_", t))
            return rc;
    }
    return 0;
}

// The bispectra table: '#' lines (npix, angle, source redshifts, the bin edges in multipoles, column names), then per
// triple i j k, the mean multipole of each of its bins, the number of closed triangles (the device's sum, rounded) and B
// of every source (%.17g; nan for a triple without a closed triangle).  One handle, one source after the other.
int LensingOutputs::bispectra()
{
    const char *who = "slicer_amd: --bispectrum";
    const int S = (int)plan.zs.size(), B = (int)o.bispectrum_edges.size() - 1;
    const size_t n = bispectrum_triples.size() / 3;
    vector<double> b(S * n), triangles(n), mean(B);
    vector<int64_t> counts(B);
    if (slicer_power_bins(p.npix, B + 1, o.bispectrum_edges.data(), counts.data(), mean.data()) != SLICER_OK)
        return fail(nullptr, who);
    for (int s = 0; s < S; s++) {
        float *d_kappa = nullptr;
        if (slicer_kappa_device_map(kh, s, &d_kappa) != SLICER_OK || slicer_bispectrum_run(bsh, d_kappa) != SLICER_OK ||
            slicer_bispectrum_read(bsh, &b[s * n], triangles.data(), nullptr) != SLICER_OK)
            return fail(h, who);
    }
    const double ell_f = 2.0 * M_PI / (p.fov * M_PI / 180.0);
    string bl;
    add(bl, "# npix %d\n# angle_deg %.17g\n# zs", p.npix, p.fov);
    for (double z : plan.zs)
        add(bl, " %.17g", z);
    add(bl, "\n# ell_edges");
    for (double r : o.bispectrum_edges)
        add(bl, " %.17g", r * ell_f);
    add(bl, "\n# i j k ell_mean_i ell_mean_j ell_mean_k n_triangles");
    for (int s = 0; s < S; s++)
        add(bl, " B_%d", s);
    add(bl, "\n");
    for (size_t t = 0; t < n; t++) {
        const int32_t *r = &bispectrum_triples[3 * t];
        add(bl, "%d %d %d %.17g %.17g %.17g %lld", (int)r[0], (int)r[1], (int)r[2], ell_f * mean[r[0]], ell_f * mean[r[1]],
            ell_f * mean[r[2]], (long long)llrint(triangles[t]));
        for (int s = 0; s < S; s++)
            add(bl, " %.17g", b[s * n + t]);
        add(bl, "\n");
    }
    return write_table("bispectra", ".bl_", bl);
}

// "Saving the <what> on:" <directory><simulation><token><npix>_<suffix>.txt, then the file; 0, or 1 after the message
int LensingOutputs::write_table(const char *what, const char *token, const string &text) const
{
    const string path = p.directory + p.simulation + token + p.snpix + "_" + p.suffix + ".txt";
    cout << "Saving the " << what << " on: " << path << endl;
    FILE *f = fopen(path.c_str(), "w");
    if (!f) {
        cerr << "It was not possible to create the file: " << path << endl;
        return 1;
    }
    fputs(text.c_str(), f);
    if (fclose(f) != 0) {
        cerr << "It was not possible to write the file: " << path << endl;
        return 1;
    }
    return 0;
}

}  // namespace slicer_amd
