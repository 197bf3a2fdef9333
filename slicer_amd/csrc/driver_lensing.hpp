// driver_lensing.hpp -- the lensing outputs of the SLICER_amd driver (slicer_main.cpp): their options, their host
// planning and the device-0 work behind --kappa, --shear, --deflection, --raytrace, --power, --pcl, --pcl-shear, --xi, --moments, --peaks,
// --minkowski, --betti, --bispectrum, --smooth, --shape-noise, --starlet, --scattering and --catalogue (driver_lensing.cpp describes the options), with the small helpers the rest of the driver shares with them.
#pragma once
#include <deque>
#include <string>
#include <vector>

#include "fits_writer.hpp"
#include "subfile_deposit.hpp"

namespace slicer_amd {

std::string plane_label(int pll);                    // slicer-v2.cpp:154-159: pll >= 0, zero-padded to three digits
std::vector<std::string> split(const std::string &s);  // the pieces of s between commas, empty ones included

struct LensingOptions {
    std::string kappa;  // "" (no lensing output at all), "all" or "z1,z2,..."
    bool growth = true, shear = false, deflection = false, raytrace = false;
    std::string shear_derivative;     // "" (not given: fft), "fft" or "gradient"
    std::string power;                // "", "auto" or "cross"
    std::vector<double> power_edges;  // empty: the default edges 0 .. npix-1
    std::string pcl;                  // "" (no --pcl), "auto" or "cross"
    std::vector<double> pcl_edges;    // --pcl-edges, required with it: at most 513
    bool pcl_taper_given = false;
    double pcl_taper_arcmin = 0.0;    // --pcl-taper: the width of the border taper, 0 without it
    std::string pcl_mask;             // --pcl-mask: a FITS image of the map's size, "" without it
    bool pcl_shear = false;           // --pcl-shear: with --pcl and --shear, the E/B pseudo-spectra as well (at most 129 edges)
    std::string xi;                   // "" (no --xi), "auto" or "cross"
    std::vector<double> xi_edges;     // --xi-edges in arcminutes, required with it: at most 513
    std::string xi_mask;              // --xi-mask: a FITS image of the map's size, "" without it
    bool moments = false, moments_levels_given = false;
    int moments_levels = 0;
    std::vector<double> peaks_edges;  // empty: no --peaks
    std::vector<double> minkowski_thresholds;  // empty: no --minkowski
    std::vector<double> betti_thresholds;      // empty: no --betti
    std::string bispectrum;                 // "" (no --bispectrum), "all" or "equilateral"
    std::vector<double> bispectrum_edges;   // --bispectrum-edges, required with it: at most 33
    std::string smooth_kind;             // "" (no --smooth), "gauss" or "map"
    std::vector<double> smooth_arcmin;   // its scales
    bool shape_noise = false;            // --shape-noise sigma_e,ngal[,seed[,nreal]]
    double noise_sigma_e = 0.0, noise_ngal = 0.0;  // per component; per arcmin^2
    uint64_t noise_seed = 0;
    int noise_nreal = 1;
    int starlet_scales = 0;              // --starlet J:lo,hi,bins: J, 0 without it
    std::vector<double> starlet_edges;   // ... the bins + 1 uniform edges from lo to hi
    int scattering_J = 0, scattering_L = 0;  // --scattering J,L: the scales and the orientations, 0 without it
    bool catalogue = false;                  // --catalogue min_peak[,capacity]
    double catalogue_min_peak = 0.0;
    int64_t catalogue_capacity = 1 << 20;    // records a map: 32 MiB on the device

    bool gradient() const { return shear_derivative == "gradient"; }
    int n_power_edges(int npix) const { return power_edges.empty() ? npix : (int)power_edges.size(); }
    const double *power_edges_or_null() const { return power_edges.empty() ? nullptr : power_edges.data(); }
    double pcl_taper_pix(int npix, double angle_deg) const { return pcl_taper_arcmin * npix / (60.0 * angle_deg); }
    // --xi-edges in pixels of a map of npix pixels and angle_deg degrees a side
    std::vector<double> xi_edges_pix(int npix, double angle_deg) const
    {
        std::vector<double> e(xi_edges);
        for (double &v : e)
            v = v * npix / (60.0 * angle_deg);
        return e;
    }
    // scale k of --smooth in pixels of a map of npix pixels and angle_deg degrees a side
    double smooth_sigma_pix(size_t k, int npix, double angle_deg) const { return smooth_arcmin[k] * npix / (60.0 * angle_deg); }

    // argv[i] with its value if it is one of these options: 0, or 2 after the message of a bad value; otherwise -1
    int parse(int argc, char **argv, int &i);
    int check() const;                           // against each other: 0, or 2 after the first broken rule's message
    int check_npix(const InputParams &p) const;  // against the map size, on the host: 0, or 2 after the message
};

// What the host works out before any device is opened (0, or the exit status after the message).  Without --kappa,
// zs stays empty.
struct LensingPlan {
    std::vector<double> zs, coeff;  // source redshifts; coeff[s * nplanes + i] = c[s][i] (slicer_lensing_weights)
    // --raytrace (slicer_lensing_plane_strengths): per plane its strength and distance, per source its distance and the
    // number of planes in front of it
    std::vector<double> strength, chil, chis;
    std::vector<int32_t> in_front;
};
int plan_lensing(const LensingOptions &o, const InputParams &p, const Header &simdata, const Lens &lens, LensingPlan &plan);

// A sub-handle of the root handle and the call that releases it.
template <class H, int (*Destroy)(H)>
struct Owned {
    H handle = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (handle) Destroy(handle); }
    operator H() const { return handle; }
    H *out() { return &handle; }
};

// npix^2 f32 device buffers of the root handle, freed in the order they were made
struct DeviceMaps {
    const slicer_handle h;
    std::vector<float *> maps{};
    explicit DeviceMaps(slicer_handle h_) : h(h_) {}
    DeviceMaps(const DeviceMaps &) = delete;
    DeviceMaps &operator=(const DeviceMaps &) = delete;
    ~DeviceMaps()
    {
        for (float *b : maps)
            slicer_device_free(h, b);
    }
    bool add(int npix)  // false: slicer_last_error(h) says why
    {
        void *b = nullptr;
        if (slicer_device_malloc(h, (size_t)npix * (size_t)npix * sizeof(float), &b) == SLICER_OK)
            maps.push_back((float *)b);
        return b != nullptr;
    }
};

// The kappa maps and what is computed from them, on the root handle.  Declared after the Ranks, so that it is released
// before its parent handle.  The members are in the order of their creation: they are released last to first.
struct LensingOutputs {
    const slicer_handle h;
    const LensingOptions &o;
    const LensingPlan &plan;
    const InputParams &p;
    const Lens &lens;
    Owned<slicer_kappa_handle, slicer_kappa_destroy> kh{};  // null without --kappa, and then all below are unused
    Owned<slicer_shear_handle, slicer_shear_destroy> shh{};  // --shear and --raytrace
    Owned<slicer_power_handle, slicer_power_destroy> ph{};
    Owned<slicer_pcl_handle, slicer_pcl_destroy> pclh{};  // --pcl
    // --pcl-shear: every source a field (gamma1, gamma2, kappa); the device copies of each source's gammas, made as
    // they are written (the shear handle keeps one source's at a time)
    Owned<slicer_pcl2_handle, slicer_pcl2_destroy> pcl2h{};
    DeviceMaps pcl2_gamma{h};
    // --xi: the kappa maps' handle (spin 0, every source a field) and with --shear a spin-2 one of one field, run as
    // each source's shear is made; the rows of the .xipm_ table, [source][bin] of (xi+, xi-)
    Owned<slicer_xi_handle, slicer_xi_destroy> xih{}, xipmh{};
    std::vector<double> xipm_rows{};
    Owned<slicer_moments_handle, slicer_moments_destroy> mh{};
    Owned<slicer_peaks_handle, slicer_peaks_destroy> pkh{};
    Owned<slicer_minkowski_handle, slicer_minkowski_destroy> mkh{};
    Owned<slicer_betti_handle, slicer_betti_destroy> bth{};
    Owned<slicer_bispectrum_handle, slicer_bispectrum_destroy> bsh{};  // --bispectrum: one handle, source after source
    std::vector<int32_t> bispectrum_triples{};                         // its list, rows (i, j, k)
    std::deque<Owned<slicer_smooth_handle, slicer_smooth_destroy>> smh{};  // --smooth: one per scale
    std::vector<int32_t> smooth_radius{};
    // --shape-noise: one handle for all sources, the noise of a pixel, the gain of every --smooth scale on it, and the
    // stream of every source: its rank in ascending redshift, so that the order of the --kappa list changes no file
    Owned<slicer_noise_handle, slicer_noise_destroy> nh{};
    double noise_sigma_pix = 0.0;
    std::vector<double> noise_gain{};
    std::vector<uint32_t> noise_stream{};
    // --starlet: one transform handle for all sources; the gains [J + 1] (the coarse map's, then w_1 ... w_J); the edges
    // of the tables with a peaks and an l1norm handle on them: one set in kappa units, or with --shape-noise one per
    // scale j = 1 ... J in units of sigma_j = noise_sigma_pix * gain_j.  The tables: peaks and l1, of the kappa and of
    // the noisy maps
    Owned<slicer_starlet_handle, slicer_starlet_destroy> sth{};
    std::vector<double> starlet_gain{}, starlet_sigma{};
    std::vector<std::vector<double>> starlet_scale_edges{};
    std::deque<Owned<slicer_peaks_handle, slicer_peaks_destroy>> starlet_pkh{};
    std::deque<Owned<slicer_l1norm_handle, slicer_l1norm_destroy>> starlet_l1h{};
    std::string starlet_tables[2][2]{};
    // --scattering: one handle for all sources; the tables of the kappa and of the noisy maps
    Owned<slicer_scattering_handle, slicer_scattering_destroy> sch{};
    std::string scattering_tables[2]{};
    // --catalogue: one handle for every map, the host copy of a map's records, the table of every kind of map
    Owned<slicer_catalogue_handle, slicer_catalogue_destroy> cth{};
    std::vector<slicer_catalogue_record> catalogue_records{};
    // --raytrace: a one-source kappa handle that makes a plane's lens map, the rays, their six output buffers, and the
    // sources in ascending redshift with the position of the next one to observe
    Owned<slicer_kappa_handle, slicer_kappa_destroy> lkh{};
    Owned<slicer_rays_handle, slicer_rays_destroy> rh{};
    DeviceMaps rt_out{h};
    std::vector<size_t> rt_order{};
    size_t rt_next = 0;
    DeviceMaps upload{h};        // planes read back from their files
    std::vector<float> map{};    // the host copy of the map that save() writes
    // The tables of --moments, --peaks, --minkowski and --betti, which write() gathers source by source: one per statistic and
    // kind of map -- the kappa maps, the smoothed ones scale by scale, the noisy ones realisation by realisation, and
    // the smoothed noisy ones
    enum Statistic { MOMENTS, PEAKS, MINKOWSKI, BETTI, N_STATISTICS };
    enum MapKind { KAPPA, SMOOTH, NOISY, NOISY_SMOOTH, N_KINDS };
    std::string tables[N_STATISTICS][N_KINDS]{};
    std::string catalogue_tables[N_KINDS]{};

    int create();
    // The planes i0 .. i1-1 of one pass go into the kappa maps as ONE batch whether they were deposited now (their
    // finalized maps on the root, plane k of `todo`) or read back from the files a previous run left (resume): the
    // batches, and with them the roundings, are the same in both cases.
    int add_pass(int i0, int i1, const std::vector<int> &todo);
    // every file of the finished kappa maps
    int write();

private:
    int trace_plane(int i, const float *d_map);
    int observe_sources(int done);
    bool save(const char *what, const std::string &token, size_t s, const std::vector<FitsKey> &more = {});
    // The rows of source s for the map at d_map onto the end of `text`, led by its '#' lines while it is empty.
    // Smoothed and noisy maps: `head` goes between the '#' lines and the column names, `lead_names` ("scale ", "real ",
    // "real scale ") in front of the column names and `lead` (their values, each followed by a blank) in front of every row.
    int source_moments(size_t s, const float *d_map, std::string &text, const std::string &head,
                       const std::string &lead_names, const std::string &lead);
    int source_peaks(size_t s, float *d_map, std::string &text, const std::string &head, const std::string &lead_names,
                     const std::string &lead);
    int source_minkowski(size_t s, float *d_map, std::string &text, const std::string &head, const std::string &lead_names,
                         const std::string &lead);
    int source_betti(size_t s, float *d_map, std::string &text, const std::string &head, const std::string &lead_names,
                     const std::string &lead);
    // --catalogue: the peaks of the map itself (no pyramid levels), z in front of `lead`
    int source_catalogue(size_t s, const float *d_map, std::string &text, const std::string &head,
                         const std::string &lead_names, const std::string &lead);
    // ... of every statistic that is on, into its table of this kind of map: moments, then peaks, Minkowski, Betti (the
    // last three read the pyramid that the moments of the same map left behind), then the catalogue
    int map_statistics(size_t s, float *d_map, MapKind kind, const std::string &head = "", const std::string &lead_names = "",
                       const std::string &lead = "");
    // The '#' lines of a --peaks / --minkowski / --betti table while `text` is empty: npix, angle, levels, `name` and the values,
    // `head`, the column names.  The levels of the pyramid under d_map, 0 (the map itself) ... levels: rows(l, d_level).
    void counts_head(std::string &text, const char *name, const std::vector<double> &values, const std::string &head,
                     const std::string &columns) const;
    template <class Rows>
    int pyramid_levels(const char *who, float *d_map, Rows rows);
    std::string smooth_head() const;
    std::string noise_head() const;
    int source_smooth(size_t s, const float *d_kappa);
    int source_noise(size_t s, const float *d_kappa);
    // --starlet of the map at d_map of source s: the files <prefix>starlet<j>_kappa_z with `keys`, SCALE and GAIN, and
    // its rows of the two tables of the noisy (or not) maps; `lead_names` and `lead` as above
    int source_starlet(size_t s, const float *d_map, bool noisy, const std::string &prefix, const std::vector<FitsKey> &keys,
                       const std::string &lead_names, const std::string &lead);
    // --scattering of the map at d_map of source s: its rows of the table of the noisy (or not) maps
    int source_scattering(size_t s, const float *d_map, bool noisy, const std::string &lead_names, const std::string &lead);
    int source_shear(size_t s, const float *d_kappa);
    int power_spectra();
    int pseudo_spectra();
    int shear_pseudo_spectra(const float *d_mask, double taper_pix, const std::string &head);
    int correlations();
    int bispectra();
    int write_table(const char *what, const char *token, const std::string &text) const;
};

}  // namespace slicer_amd
