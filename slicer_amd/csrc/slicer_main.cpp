// slicer_main.cpp -- `SLICER_amd InputParams.ini [--devices 0-7]`: the Gadget branch of slicer-v2.cpp (:23-229) on the
// MI355X GPUs of one node, without MPI.  Planning (planner.cpp) -> plane loop -> createDensityMaps-equivalent passes
// over the C ABI -> writeMaps.  With several devices one host thread drives each GPU through its own handle: the
// sub-files of every snapshot are split over the devices in the reference's contiguous ranges (slicer-v2.cpp:162-175),
// the partial maps are summed onto device 0 in the accumulator type (slicer-v2.cpp:214-217 -> RCCL over xGMI,
// include/slicer_amd_rccl.h), and device 0's thread writes the FITS files -- byte-identical to a one-device run with
// --accum fixed64, within the f32 reorder bound otherwise.
// Differences from the reference driver, all opt-out:
//   * the planes cut from one box replication (same snapshot, same Random entry, same rcase) are built in ONE pass
//     over the snapshot (the reference re-reads and re-transforms it for each of them);   --single-plane disables
//   * nparttype* keys carry the real selected counts (the reference writes 0: densitymaps.cpp:497), which also makes
//     partinplanes runs write their per-type files;                                      --reference-counts disables
//   * --kappa all|z1,z2,... adds Born convergence maps, one FITS per source redshift, accumulated on device 0 from the
//     finalized total maps of every pass (the reference's post-processing script Lens/kslicer.py);
//     --kappa-no-growth drops its linear-growth correction.  Without --kappa the run is unchanged.
//   * --shear (with --kappa) also writes, per source, the shear maps gamma1, gamma2, |gamma| and the lensing potential
//     phi computed on device 0 from the kappa map (the reference's Lens/smr.py).
//   * --deflection (with --shear) also writes the deflection maps alpha1, alpha2 (.alpha1_z, .alpha2_z, the kappa
//     header); --shear-derivative fft|gradient (with --shear, default fft) chooses where gamma1, gamma2, |gamma| and
//     the alphas come from: the FFT filters, or smr's derivative="gradient", finite differences of phi that do not
//     wrap the map's edges.  The phi and kappa files are the same either way.
//   * --raytrace (with --kappa) also shoots one ray per pixel through the planes, near to far, on device 0 (DESIGN.md S8
//     row N11): every plane's lens map strength_p (m_p - mean m_p) is turned into its deflection, convergence and shear maps
//     (the device work of --shear --deflection, per plane; --shear-derivative gradient takes the finite-difference maps)
//     and the rays step through them at chi(zl_p).  Per source, next to the kappa file and with its header:
//     .rt_kappa_z, .rt_gamma1_z, .rt_gamma2_z, .rt_omega_z (the distortion matrix) and .rt_alpha1_z, .rt_alpha2_z (the
//     total deflection, radians).  All other files are unchanged.
//   * --power auto|cross (with --kappa) also writes <directory><simulation>.cl_<npix>_<suffix>.txt: the binned auto
//     (or auto and cross) power spectra C_l of the kappa maps, computed on device 0 (Lens/smr.py's PS without its
//     defects); --power-edges r0,r1,... sets the bin edges in units of l_f = 2 pi / ANGLE
//     (default 0, 1, ..., npix-1).
//   * --moments (with --kappa) also writes <directory><simulation>.moments_<npix>_<suffix>.txt: the raw central power
//     sums S_2 ... S_8 and the mean of every kappa map and of --moments-levels L (default 0) successive 2x2 block means
//     of it, about each level's own mean, computed on device 0 (Lens/moment.py and Lens/halve.py).
//   * --peaks lo,hi,bins (with --kappa) also writes <directory><simulation>.peaks_<npix>_<suffix>.txt: the one-point PDF
//     histogram of every kappa map and the counts of its peaks and minima by height (strictly above / below all 8
//     neighbours; the map does not wrap), over `bins` (1 ... 1024) uniform bins from lo to hi, computed on device 0;
//     with --moments also of every level of its pyramid of block means.
//   * SubFind / halo-catalogue mode (npix == 0) is not supported; with snopt > 0 and several devices every rank thread
//     draws from its own copy of the libc stream, like the reference's MPI ranks (Ranks::create).
#include <dlfcn.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <valarray>
#include <vector>

#include "../../include/slicer_amd_rccl.h"
#include "fits_writer.hpp"
#include "gadget2_reader.hpp"
#include "planner.hpp"
#include "subfile_deposit.hpp"

using namespace slicer_amd;
using std::cerr;
using std::cout;
using std::endl;
using std::string;
using std::vector;

namespace {

bool file_exists(const string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

string plane_label(int pll)  // slicer-v2.cpp:154-159: pll >= 0, zero-padded to three digits
{
    char b[16];
    snprintf(b, sizeof b, "%03d", pll);
    return b;
}

void dump_plan(const string &path, const InputParams &p, const Lens &lens, const Random &random,
               const vector<double> &snapbox, double fovradiants)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f)
        return;
    fprintf(f, "{\n \"Ds\": %.17g, \"fovradiants\": %.17g, \"nplanes\": %d, \"hydro\": %d,\n", p.Ds, fovradiants,
            lens.nplanes, (int)p.hydro);
    // the process's libc rand() stream as randomizeBox left it (31 words, oldest first): what shot-noise thinning
    // (snopt > 0) starts to draw from -- null where the C library does not expose it
    uint32_t v[31];
    if (slicer_libc_rand_state_get(v) == SLICER_OK) {
        fprintf(f, " \"libc_rand_state\": [");
        for (int i = 0; i < 31; i++)
            fprintf(f, "%u%s", v[i], i < 30 ? ", " : "],\n");
    } else {
        fprintf(f, " \"libc_rand_state\": null,\n");
    }
    fprintf(f, " \"planes\": [\n");
    for (int i = 0; i < lens.nplanes; i++) {
        fprintf(f,
                "  {\"ld\": %.17g, \"ld2\": %.17g, \"zsimlens\": %.17g, \"fromsnap\": \"%s\", \"fromsnapi\": %d, "
                "\"randomize\": %d, \"replication\": %d, \"nrepperp\": %d, \"snapbox\": %.17g, \"x0\": %.17g, \"y0\": %.17g, "
                "\"z0\": %.17g, \"face\": %d, \"sgn\": [%d, %d, %d]}%s\n",
                lens.ld[i], lens.ld2[i], lens.zsimlens[i], lens.fromsnap[i].c_str(), lens.fromsnapi[i],
                (int)lens.randomize[i], lens.replication[i], lens.nrepperp[i], snapbox[lens.fromsnapi[i]], random.x0[i],
                random.y0[i], random.z0[i], random.face[i], random.sgnX[i], random.sgnY[i], random.sgnZ[i],
                i + 1 < lens.nplanes ? "," : "");
    }
    fprintf(f, " ]\n}\n");
    fclose(f);
}

// the pieces of s between commas, empty ones included
vector<string> split(const string &s)
{
    vector<string> out;
    size_t i = 0;
    for (size_t j; (j = s.find(',', i)) != string::npos; i = j + 1)
        out.push_back(s.substr(i, j - i));
    out.push_back(s.substr(i));
    return out;
}

// "all" -> empty list with all = true; "0.5,1" -> the redshifts; false on anything else
bool parse_sources(const string &spec, bool &all, vector<double> &zs)
{
    all = spec == "all";
    if (all)
        return true;
    for (const string &tok : split(spec)) {
        char *end = nullptr;
        const double z = strtod(tok.c_str(), &end);
        if (tok.empty() || *end != '\0' || !(z >= 0))
            return false;
        zs.push_back(z);
    }
    return !zs.empty();
}

// "0-3", "0,2,5", "1": HIP device ordinals, one rank each
vector<int> parse_devices(const string &spec)
{
    vector<int> out;
    for (const string &tok : split(spec)) {
        const size_t dash = tok.find('-');
        if (dash != string::npos && dash > 0) {
            for (int d = atoi(tok.substr(0, dash).c_str()); d <= atoi(tok.substr(dash + 1).c_str()); d++)
                out.push_back(d);
        } else if (!tok.empty()) {
            out.push_back(atoi(tok.c_str()));
        }
    }
    return out;
}

// libslicer_amd_rccl.so is only needed (and only loaded) when more than one device takes part
struct RcclApi {
    void *lib = nullptr;
    int (*init_all)(slicer_rccl_comm *, int, const int *) = nullptr;
    int (*destroy)(slicer_rccl_comm) = nullptr;
    int (*plane_reduce)(slicer_handle, slicer_rccl_comm, int, int) = nullptr;  // slicer_rccl_plane_reduce_ex
    const char *(*last_error)(void) = nullptr;
    bool load()
    {
        lib = dlopen("libslicer_amd_rccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) {
            cerr << "slicer_amd: " << dlerror() << endl;
            return false;
        }
        init_all = (decltype(init_all))dlsym(lib, "slicer_rccl_comm_init_all");
        destroy = (decltype(destroy))dlsym(lib, "slicer_rccl_comm_destroy");
        plane_reduce = (decltype(plane_reduce))dlsym(lib, "slicer_rccl_plane_reduce_ex");
        last_error = (decltype(last_error))dlsym(lib, "slicer_rccl_last_error");
        return init_all && destroy && plane_reduce && last_error;
    }
};

// All rank threads of a pass meet here after their deposits and learn whether any of them failed: a collective is
// entered by every rank or by none (a rank that skipped it alone would leave the others waiting in RCCL for ever; the
// reference calls MPI_Abort in that situation, slicer-v2.cpp:204-207).  One per pass.
class Rendezvous {
    std::mutex m;
    std::condition_variable cv;
    const int n;
    int waiting = 0;
    bool failed = false;

public:
    explicit Rendezvous(int n_) : n(n_) {}
    bool any_failed(bool mine)  // blocks until all n ranks have called; the same answer for all of them
    {
        std::unique_lock<std::mutex> lk(m);
        failed = failed || mine;
        if (++waiting == n)
            cv.notify_all();
        else
            cv.wait(lk, [&] { return waiting == n; });
        return failed;
    }
};

// One rank = one GPU = one handle (+ its communicator).
struct Rank {
    int device = 0;
    slicer_handle h = nullptr;
    slicer_rccl_comm comm = nullptr;
};

// The rank sum without RCCL (--reduce host): accumulators through host memory, summed in their own type onto rank 0.
// The same protocol as slicer_rccl_plane_reduce (include/slicer_amd.h "cross-rank sum"); it exists so that the
// multi-rank driver can be exercised where the ranks cannot form an RCCL clique (two handles on one GPU in the tests).
int host_plane_reduce(vector<Rank> &ranks, int npix, int n_planes)
{
    slicer_reduce_meta comb;
    for (int i = 0; i < SLICER_REDUCE_META_INTS; i++)
        comb.v[i] = INT32_MIN;
    for (auto &r : ranks) {
        slicer_reduce_meta m;
        if (slicer_reduce_meta_get(r.h, &m) != SLICER_OK)
            return fail(r.h, "slicer_amd");
        for (int i = 0; i < SLICER_REDUCE_META_INTS; i++)
            comb.v[i] = std::max(comb.v[i], m.v[i]);
    }
    for (auto &r : ranks)
        if (slicer_reduce_meta_set(r.h, &comb) != SLICER_OK)
            return fail(r.h, "slicer_amd");
    const size_t n = (size_t)npix * (size_t)npix;
    vector<unsigned char> sum, part;
    for (int p = 0; p < n_planes; p++) {
        void *acc0[7];
        int32_t elem = 0;
        if (slicer_plane_accumulators(ranks[0].h, p, acc0, &elem) != SLICER_OK)
            return 1;
        const size_t esz = elem == SLICER_ELEM_F32 ? 4 : 8;
        for (int s = 0; s < 7; s++) {
            if (!acc0[s])
                continue;
            sum.resize(n * esz);
            part.resize(n * esz);
            if (slicer_copy_to_host(ranks[0].h, sum.data(), acc0[s], n * esz) != SLICER_OK)
                return 1;
            for (size_t k = 1; k < ranks.size(); k++) {
                void *acc[7];
                int32_t e2 = 0;
                if (slicer_plane_accumulators(ranks[k].h, p, acc, &e2) != SLICER_OK || e2 != elem || !acc[s] ||
                    slicer_copy_to_host(ranks[k].h, part.data(), acc[s], n * esz) != SLICER_OK)
                    return 1;
                if (elem == SLICER_ELEM_F32) {
                    float *a = (float *)sum.data();
                    const float *b = (const float *)part.data();
                    for (size_t i = 0; i < n; i++)
                        a[i] = a[i] + b[i];
                } else if (elem == SLICER_ELEM_F64) {
                    double *a = (double *)sum.data();
                    const double *b = (const double *)part.data();
                    for (size_t i = 0; i < n; i++)
                        a[i] = a[i] + b[i];
                } else {
                    uint64_t *a = (uint64_t *)sum.data();
                    const uint64_t *b = (const uint64_t *)part.data();
                    for (size_t i = 0; i < n; i++)
                        a[i] += b[i];
                }
            }
            if (slicer_copy_to_device(ranks[0].h, acc0[s], sum.data(), n * esz) != SLICER_OK)
                return 1;
        }
        uint64_t *c0 = nullptr, tot[6], one[6];
        if (slicer_plane_device_counts(ranks[0].h, p, &c0) != SLICER_OK ||
            slicer_copy_to_host(ranks[0].h, tot, c0, sizeof tot) != SLICER_OK)
            return 1;
        for (size_t k = 1; k < ranks.size(); k++) {
            uint64_t *ck = nullptr;
            if (slicer_plane_device_counts(ranks[k].h, p, &ck) != SLICER_OK ||
                slicer_copy_to_host(ranks[k].h, one, ck, sizeof one) != SLICER_OK)
                return 1;
            for (int t = 0; t < 6; t++)
                tot[t] += one[t];
        }
        if (slicer_copy_to_device(ranks[0].h, c0, tot, sizeof tot) != SLICER_OK)
            return 1;
    }
    return 0;
}

struct Options {
    string inifile, plan_path, devices_spec, reduce_mode = "rccl", reduce_algo = "rooted", kappa_spec;
    bool kappa_growth = true, shear = false, deflection = false, raytrace = false;
    string shear_derivative;     // "" (not given: fft), "fft" or "gradient"
    string power;                // "", "auto" or "cross"
    vector<double> power_edges;  // empty: the default edges
    bool moments = false, moments_levels_given = false;
    int moments_levels = 0;
    vector<double> peaks_edges;  // empty: no --peaks
    int device = 0, mas = SLICER_MAS_TSC, accum = SLICER_ACC_F32;
    bool plan_only = false, single_plane = false, reference_counts = false, replication = false;
};

// 0, or the exit status of a bad command line
int parse_args(int argc, char **argv, Options &o)
{
    for (int i = 1; i < argc; i++) {
        string a = argv[i];
        if (a == "--device" && i + 1 < argc) o.device = atoi(argv[++i]);
        else if (a == "--devices" && i + 1 < argc) o.devices_spec = argv[++i];
        else if (a == "--reduce" && i + 1 < argc) o.reduce_mode = argv[++i];  // rccl (default) | host
        else if (a == "--reduce-algo" && i + 1 < argc) o.reduce_algo = argv[++i];  // rooted (default) | direct
        else if (a == "--ngp") o.mas = SLICER_MAS_NGP;
        else if (a == "--accum" && i + 1 < argc) {
            string v = argv[++i];
            o.accum = v == "f64" ? SLICER_ACC_F64 : (v == "fixed64" ? SLICER_ACC_FIXED64 : SLICER_ACC_F32);
        } else if (a == "--plan-only") o.plan_only = true;
        else if (a == "--dump-plan" && i + 1 < argc) o.plan_path = argv[++i];
        else if (a == "--single-plane") o.single_plane = true;
        else if (a == "--reference-counts") o.reference_counts = true;
        else if (a == "--replication") o.replication = true;  // -DUSE_REPLICATION (ReplicationOnPerpendicularPlane)
        else if (a == "--kappa" && i + 1 < argc) o.kappa_spec = argv[++i];  // all | z1,z2,...
        else if (a == "--kappa-no-growth") o.kappa_growth = false;
        else if (a == "--shear") o.shear = true;
        else if (a == "--deflection") o.deflection = true;
        else if (a == "--raytrace") o.raytrace = true;
        else if (a == "--shear-derivative" && i + 1 < argc) o.shear_derivative = argv[++i];  // fft | gradient
        else if (a == "--power" && i + 1 < argc) o.power = argv[++i];  // auto | cross
        else if (a == "--power-edges" && i + 1 < argc) {
            for (const string &tok : split(argv[++i])) {
                char *end = nullptr;
                const double r = strtod(tok.c_str(), &end);
                if (tok.empty() || *end != '\0') {
                    cerr << "bad --power-edges (a comma-separated list of radii in units of l_f)" << endl;
                    return 2;
                }
                o.power_edges.push_back(r);
            }
        }
        else if (a == "--moments") o.moments = true;
        else if (a == "--moments-levels") {
            if (i + 1 >= argc) {
                cerr << "--moments-levels needs a value (the number of halvings below the kappa map)" << endl;
                return 2;
            }
            char *end = nullptr;
            const long v = strtol(argv[++i], &end, 10);
            if (end == argv[i] || *end != '\0' || v < -1000 || v > 1000) {
                cerr << "bad --moments-levels (the number of halvings below the kappa map)" << endl;
                return 2;
            }
            o.moments_levels = (int)v;
            o.moments_levels_given = true;
        }
        else if (a == "--peaks") {
            const vector<string> tok = i + 1 < argc ? split(argv[++i]) : vector<string>{};
            char *e0 = nullptr, *e1 = nullptr, *e2 = nullptr;
            const double lo = tok.size() == 3 ? strtod(tok[0].c_str(), &e0) : 0.0;
            const double hi = tok.size() == 3 ? strtod(tok[1].c_str(), &e1) : 0.0;
            const long bins = tok.size() == 3 ? strtol(tok[2].c_str(), &e2, 10) : 0;
            if (tok.size() != 3 || tok[0].empty() || tok[1].empty() || tok[2].empty() || *e0 != '\0' || *e1 != '\0' ||
                *e2 != '\0' || bins < 1 || bins > SLICER_PEAKS_MAX_BINS) {
                cerr << "bad --peaks (lo,hi,bins: the first and the last edge and the number of bins, 1 ... "
                     << SLICER_PEAKS_MAX_BINS << ")" << endl;
                return 2;
            }
            o.peaks_edges.resize(bins + 1);
            if (slicer_peaks_edges(lo, hi, (int32_t)bins, o.peaks_edges.data()) != SLICER_OK) {
                cerr << "bad --peaks: " << slicer_last_error(nullptr) << endl;
                return 2;
            }
        }
        else if (o.inifile.empty()) o.inifile = a;
        else {
            cerr << "unknown argument " << a << endl;
            return 2;
        }
    }
    if (o.inifile.empty()) {
        cout << "No params!! Nothing to be done!" << endl;  // slicer-v2.cpp:34
        return 2;
    }
    if (o.shear && o.kappa_spec.empty()) {
        cerr << "--shear needs --kappa (the shear maps are computed from the kappa maps)" << endl;
        return 2;
    }
    if (o.raytrace && o.kappa_spec.empty()) {
        cerr << "--raytrace needs --kappa (the rays are observed at the source redshifts of the kappa maps)" << endl;
        return 2;
    }
    if (o.deflection && !o.shear) {
        cerr << "--deflection needs --shear (the deflection maps are computed from the spectrum of the shear maps)" << endl;
        return 2;
    }
    if (!o.shear_derivative.empty() && o.shear_derivative != "fft" && o.shear_derivative != "gradient") {
        cerr << "bad --shear-derivative (fft or gradient)" << endl;
        return 2;
    }
    if (!o.shear_derivative.empty() && !o.shear && !o.raytrace) {
        cerr << "--shear-derivative needs --shear" << endl;
        return 2;
    }
    if (!o.power.empty() && o.power != "auto" && o.power != "cross") {
        cerr << "bad --power (auto or cross)" << endl;
        return 2;
    }
    if (!o.power.empty() && o.kappa_spec.empty()) {
        cerr << "--power needs --kappa (the power spectra are those of the kappa maps)" << endl;
        return 2;
    }
    if (!o.power_edges.empty() && o.power.empty()) {
        cerr << "--power-edges needs --power" << endl;
        return 2;
    }
    if (o.moments && o.kappa_spec.empty()) {
        cerr << "--moments needs --kappa (the moments are those of the kappa maps)" << endl;
        return 2;
    }
    if (o.moments_levels_given && !o.moments) {
        cerr << "--moments-levels needs --moments" << endl;
        return 2;
    }
    if (!o.peaks_edges.empty() && o.kappa_spec.empty()) {
        cerr << "--peaks needs --kappa (the histograms and peak counts are those of the kappa maps)" << endl;
        return 2;
    }
    return 0;
}

constexpr int myid = 0;  // one process: the reference's rank 0

// the header of sub-file 0 of snapshot File; false after the reference's message
bool read_header(const string &File, Header &hdr)
{
    SnapshotFile s0;
    if (!s0.open(File + ".0")) {
        cerr << "Error in opening the file: " << File + ".0" << "!\n\a";
        return false;
    }
    hdr = s0.header();
    return true;
}

// The light cone as slicer-v2.cpp:30-135 plans it.
struct Cone {
    InputParams p{};
    Header simdata{};  // of the first snapshot's sub-file 0
    vector<double> snapbox;
    NaturalCubicSpline getZl;
    Lens lens{};
    Random random;
    double fovradiants = 0;
};

// readInput ... randomizeBox, then --dump-plan; 0, or the exit status
int plan_cone(const Options &o, Cone &c)
{
    InputParams &p = c.p;
    if (readInput(p, o.inifile))
        return 1;
    if (o.shear && !slicer_shear_supported(p.npix)) {
        cerr << "--shear: npix = " << p.npix << " is not supported (2 ... 16384, prime factors 2, 3, 5, 7 only)" << endl;
        return 2;
    }
    if (o.raytrace && !p.physical && !slicer_shear_supported(p.npix)) {  // (physical: refused with the weights)
        cerr << "--raytrace: npix = " << p.npix << " is not supported (2 ... 16384, prime factors 2, 3, 5, 7 only)" << endl;
        return 2;
    }
    if (o.shear_derivative == "gradient" && p.npix < 5) {
        cerr << "--shear-derivative gradient: npix = " << p.npix << " is not supported (the stencils take at least 5)" << endl;
        return 2;
    }
    if (!o.power.empty() && !slicer_shear_supported(p.npix)) {
        cerr << "--power: npix = " << p.npix << " is not supported (2 ... 16384, prime factors 2, 3, 5, 7 only)" << endl;
        return 2;
    }
    if (!o.power.empty()) {  // the edges, checked on the host before any device work
        const int ne = o.power_edges.empty() ? p.npix : (int)o.power_edges.size();
        vector<int64_t> cnt(std::max(ne - 1, 1));
        vector<double> mr(cnt.size());
        if (slicer_power_bins(p.npix, ne, o.power_edges.empty() ? nullptr : o.power_edges.data(), cnt.data(),
                              mr.data()) != SLICER_OK) {
            cerr << "--power-edges: " << slicer_last_error(nullptr) << endl;
            return 2;
        }
    }
    if (o.moments) {  // the pyramid's depth, checked on the host before any device work
        int most = 0;
        while (p.npix >> (most + 1) > 0)
            most++;
        if (p.npix < 1 || o.moments_levels < 0 || o.moments_levels > most) {
            cerr << "--moments-levels " << o.moments_levels << " is outside 0 ... " << most << " = floor(log2 npix) for npix = "
                 << p.npix << endl;
            return 2;
        }
    }
    if (p.simType == "SubFind") {
        cerr << "SubFind / halo light-cone mode (npix == 0) is outside this driver's scope" << endl;
        return 1;
    }
    vector<string> snappath;
    vector<double> snapred;
    if (readRedList(p.filredshiftlist, snapred, snappath, c.snapbox, p))
        return 1;
    if (!read_header(p.pathsnap + snappath[0], c.simdata))
        return 1;
    testHydro(p, c.simdata);

    // slicer-v2.cpp:79-96: distance table (h = 1) and the two interpolators
    const Cosmology cosmo{100.0, c.simdata.om0, c.simdata.oml, p.w, 0.0};
    vector<double> zl(kNeval);
    for (int i = 0; i < kNeval; i++)
        zl[i] = i * (p.zs + 1.0) / (kNeval - 1);
    vector<double> dl;
    try {
        dl = transverseDistanceTable(cosmo, zl);
    } catch (const std::exception &e) {
        cerr << e.what() << endl;
        return 1;
    }
    NaturalCubicSpline getDl;
    getDl.init(zl, dl);
    c.getZl.init(dl, zl);
    p.Ds = getDl.eval(p.zs);

    Lens &lens = c.lens;
    if (buildPlanes(p, lens, snapred, snappath, c.snapbox, getDl, c.getZl, kNumberOfLensPerSnap, myid))
        return 1;
    lens.nrepperp.resize(lens.ld.size(), 0);
    for (size_t i = 0; i < lens.ld.size(); i++) {  // slicer-v2.cpp:103-125
        const double boxl = c.snapbox[lens.fromsnapi[i]] / 1e3 * kPosU;
        if (!o.replication) {
            if (testFov(p.fov, boxl, lens.ld2[i], myid, c.fovradiants))
                return 1;
        } else {
            computeReplications(p.fov, boxl, lens.ld2[i], myid, c.fovradiants, lens.nrepperp[i]);
        }
    }
    randomizeBox(c.random, lens, p, kNumberOfLensPerSnap, myid);
    if (!o.plan_path.empty())
        dump_plan(o.plan_path, p, lens, c.random, c.snapbox, c.fovradiants);
    return 0;
}

// Born convergence maps: weights c[s][p] for every plane of the cone (slicer_lensing_weights), before any GPU work.
// Without --kappa, zs stays empty.  0, or the exit status
int kappa_weights(const Options &o, const Cone &c, vector<double> &zs, vector<double> &coeff)
{
    if (o.kappa_spec.empty())
        return 0;
    bool all = false;
    if (!parse_sources(o.kappa_spec, all, zs)) {
        cerr << "bad --kappa (all, or a comma-separated list of source redshifts)" << endl;
        return 2;
    }
    const int P = c.lens.nplanes;
    vector<double> zup(P);
    const int S = all ? P : (int)zs.size();
    coeff.assign((size_t)S * P, 0.0);
    if (slicer_lensing_weights(c.simdata.om0, c.simdata.oml, c.p.w, 0.0, c.p.fov, c.p.npix, o.kappa_growth, c.p.physical,
                               P, c.lens.ld.data(), c.lens.ld2.data(), c.lens.zfromsnap.data(), S,
                               all ? nullptr : zs.data(), coeff.data(), nullptr, zup.data(), nullptr, nullptr) != SLICER_OK)
        return fail(nullptr, "slicer_amd: --kappa");
    if (all)
        zs = zup;
    return 0;
}

// --raytrace: the strength and distance of every plane, the distance of every source and the number of planes in front of
// it (slicer_lensing_plane_strengths), before any GPU work.  0, or the exit status
struct RayPlan {
    vector<double> strength, chil, chis;
    vector<int32_t> in_front;
};
int raytrace_plan(const Options &o, const Cone &c, const vector<double> &zs, RayPlan &rp)
{
    if (!o.raytrace)
        return 0;
    const int P = c.lens.nplanes, S = (int)zs.size();
    rp.strength.resize(P);
    rp.chil.resize(P);
    rp.chis.resize(S);
    rp.in_front.resize(S);
    if (slicer_lensing_plane_strengths(c.simdata.om0, c.simdata.oml, c.p.w, 0.0, c.p.fov, c.p.npix, o.kappa_growth,
                                       c.p.physical, P, c.lens.ld.data(), c.lens.ld2.data(), c.lens.zfromsnap.data(), S,
                                       zs.data(), rp.strength.data(), rp.chil.data(), rp.chis.data(),
                                       rp.in_front.data()) != SLICER_OK)
        return fail(nullptr, "slicer_amd: --raytrace");
    for (int i = 1; i < P; i++)
        if (!(rp.chil[i] > rp.chil[i - 1])) {
            cerr << "--raytrace: the plane distances are not strictly ascending (plane " << i << " at " << rp.chil[i]
                 << " after " << rp.chil[i - 1] << " Mpc/h)" << endl;
            return 2;
        }
    return 0;
}

// The ranks of the run: one handle per device, their copies of the libc rand() stream and, with several devices and
// --reduce rccl, their communicators.  The destructor releases them.
struct Ranks {
    vector<Rank> r;
    RcclApi rccl;

    ~Ranks()
    {
        for (auto &R : r) {
            if (R.comm)
                rccl.destroy(R.comm);
            slicer_destroy(R.h);
        }
    }
    // device 0 of the list is the root: it ends up with the sums and writes the maps
    slicer_handle root() const { return r[0].h; }

    // snopt > 0: the reference's MPI ranks each own an identically seeded copy of libc's rand() stream (randomizeBox
    // seeds it in every rank alike) and consume it independently (densitymaps.cpp:387-397).  Rank threads would
    // interleave their draws on the one process-global stream, and the HIP runtime's own threads call rand() at
    // unpredictable points once it runs (code-object loading, ...).  So the stream is read here, before the first HIP
    // call, and every handle thins from a copy of its own -- the run then equals a reference run on as many MPI ranks.
    // Where that state cannot be read (no glibc TYPE_3 generator), several devices are refused.
    int create(const vector<int> &devs, int snopt, bool use_rccl)
    {
        uint32_t stream[31];
        bool private_streams = snopt != 0;
        if (private_streams && slicer_libc_rand_state_get(stream) != SLICER_OK) {
            if (devs.size() > 1) {
                cerr << "snopt > 0 on several devices needs per-rank copies of the libc rand() stream, which this C "
                        "library does not expose (slicer_libc_rand_supported() == 0): use a single device" << endl;
                return 2;
            }
            private_streams = false;  // one device: the process-global stream, drawn with rand() on the host
        }
        r.resize(devs.size());
        for (size_t k = 0; k < devs.size(); k++) {
            r[k].device = devs[k];
            if (slicer_create(devs[k], 1ull << 24, &r[k].h) != SLICER_OK)
                return fail(nullptr, "slicer_amd");
            if (private_streams && slicer_rand_stream_set(r[k].h, stream) != SLICER_OK)
                return fail(r[k].h, "slicer_amd");
        }
        const int n = (int)r.size();
        if (n > 1 && use_rccl) {
            vector<slicer_rccl_comm> comms(n);
            if (!rccl.load() || rccl.init_all(comms.data(), n, devs.data()) != SLICER_OK) {
                cerr << "slicer_amd: cannot set up RCCL over the devices: " << (rccl.last_error ? rccl.last_error() : "")
                     << endl;
                return 1;
            }
            for (int k = 0; k < n; k++)
                r[k].comm = comms[k];
        }
        return 0;
    }
};

// --kappa / --shear / --power / --moments / --peaks: the kappa maps, and the shear maps, power spectra, moments and
// histograms computed from them, on the root handle.  Declared after the Ranks, so that it is released before its parent handle.
struct LensingOutputs {
    const slicer_handle h;
    const InputParams &p;
    const Lens &lens;
    const vector<double> &zs, &coeff;  // source redshifts; coeff[s * nplanes + i] = c[s][i] (kappa_weights)
    slicer_kappa_handle kh = nullptr;  // nullptr without --kappa
    slicer_shear_handle shh = nullptr;
    slicer_power_handle ph = nullptr;
    slicer_moments_handle mh = nullptr;
    int moments_levels = -1;  // -1: no --moments
    slicer_peaks_handle pkh = nullptr;
    vector<double> peaks_edges{};  // empty: no --peaks
    bool deflection = false, gradient = false;  // --deflection; --shear-derivative gradient
    string power_mode{};           // "", "auto" or "cross"
    vector<double> power_edges{};  // empty: 0 .. npix-1
    vector<float *> upload{};  // device buffers for planes read back from their files
    bool shear_files = false;  // --shear: the shear handle's maps of every kappa map are written
    // --raytrace: the plan, a one-source kappa handle that makes a plane's lens map, the rays, their six output buffers,
    // and the sources in ascending redshift with the position of the next one to observe
    const RayPlan *rt = nullptr;
    slicer_kappa_handle lkh = nullptr;
    slicer_rays_handle rh = nullptr;
    float *rt_out[SLICER_RAYS_COUNT] = {};
    vector<size_t> rt_order{};
    size_t rt_next = 0;

    ~LensingOutputs()
    {
        for (float *b : upload)
            slicer_device_free(h, b);
        for (float *b : rt_out)
            if (b)
                slicer_device_free(h, b);
        if (rh)
            slicer_rays_destroy(rh);
        if (lkh)
            slicer_kappa_destroy(lkh);
        if (pkh)
            slicer_peaks_destroy(pkh);
        if (mh)
            slicer_moments_destroy(mh);
        if (ph)
            slicer_power_destroy(ph);
        if (shh)
            slicer_shear_destroy(shh);
        if (kh)
            slicer_kappa_destroy(kh);
    }

    int create(bool shear)
    {
        if (!zs.empty() && slicer_kappa_create(h, p.npix, (int)zs.size(), &kh) != SLICER_OK)
            return fail(h, "slicer_amd: --kappa");
        shear_files = kh && shear;
        if (kh && (shear || rt) && slicer_shear_create(h, p.npix, p.fov, &shh) != SLICER_OK)
            return fail(h, "slicer_amd: --shear");
        if (kh && !power_mode.empty()) {
            const int ne = power_edges.empty() ? p.npix : (int)power_edges.size();
            if ((int)zs.size() > 128) {
                cerr << "slicer_amd: --power: " << zs.size() << " sources, at most 128" << endl;
                return 2;
            }
            if (slicer_power_create(h, p.npix, p.fov, (int)zs.size(), power_mode == "cross", ne,
                                    power_edges.empty() ? nullptr : power_edges.data(), &ph) != SLICER_OK)
                return fail(h, "slicer_amd: --power");
        }
        if (kh && moments_levels >= 0 &&
            slicer_moments_create(h, p.npix, moments_levels, SLICER_HALVE_MEAN, &mh) != SLICER_OK)
            return fail(h, "slicer_amd: --moments");
        if (kh && !peaks_edges.empty() &&
            slicer_peaks_create(h, p.npix, (int)peaks_edges.size(), peaks_edges.data(), &pkh) != SLICER_OK)
            return fail(h, "slicer_amd: --peaks");
        if (kh && rt) {
            if (slicer_kappa_create(h, p.npix, 1, &lkh) != SLICER_OK ||
                slicer_rays_create(h, p.npix, p.fov * M_PI / 180.0 / p.npix, &rh) != SLICER_OK)
                return fail(h, "slicer_amd: --raytrace");
            for (float *&b : rt_out)
                if (slicer_device_malloc(h, (size_t)p.npix * (size_t)p.npix * sizeof(float), (void **)&b) != SLICER_OK)
                    return fail(h, "slicer_amd: --raytrace");
            rt_order.resize(zs.size());
            for (size_t s = 0; s < zs.size(); s++)
                rt_order[s] = s;
            std::stable_sort(rt_order.begin(), rt_order.end(), [&](size_t a, size_t b) { return zs[a] < zs[b]; });
            return observe_sources(0);  // the sources with no plane in front: from the start state
        }
        return 0;
    }

    // --raytrace, plane i of the cone, whose mass map is d_map: its lens map L = strength (m - mean m) from the one-source
    // kappa handle, the maps of L from the shear handle, one step of the rays, and the sources this plane is the last
    // in front of.
    int trace_plane(int i, const float *d_map)
    {
        const char *who = "slicer_amd: --raytrace";
        float *L = nullptr, *m[5] = {};
        const int spectral[5] = {SLICER_SHEAR_ALPHA1, SLICER_SHEAR_ALPHA2, -1, SLICER_SHEAR_GAMMA1, SLICER_SHEAR_GAMMA2};
        const int fd[5] = {SLICER_SHEAR_FD_ALPHA1, SLICER_SHEAR_FD_ALPHA2, SLICER_SHEAR_FD_KAPPA, SLICER_SHEAR_FD_GAMMA1,
                           SLICER_SHEAR_FD_GAMMA2};
        if (slicer_kappa_add(lkh, 1, &d_map, &rt->strength[i]) != SLICER_OK || slicer_kappa_finalize(lkh) != SLICER_OK ||
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
        if (slicer_rays_step(rh, rt->chil[i], m[0], m[1], m[2], m[3], m[4]) != SLICER_OK ||
            slicer_kappa_reset(lkh) != SLICER_OK)
            return fail(h, who);
        return observe_sources(i + 1);
    }

    // the sources, in ascending redshift, that have `done` planes in front of them: observed now and written
    int observe_sources(int done)
    {
        static const char *const token[SLICER_RAYS_COUNT] = {".rt_kappa_z",  ".rt_gamma1_z", ".rt_gamma2_z",
                                                              ".rt_omega_z",  ".rt_alpha1_z", ".rt_alpha2_z"};
        vector<float> map((size_t)p.npix * (size_t)p.npix);
        for (; rt_next < rt_order.size() && rt->in_front[rt_order[rt_next]] <= done; rt_next++) {
            const size_t s = rt_order[rt_next];
            char zbuf[32];
            snprintf(zbuf, sizeof zbuf, "%.4f", zs[s]);
            const FitsKey keys[2] = {{"ZSOURCE", false, 0, zs[s], " "}, {"ANGLE", false, 0, p.fov, " "}};
            if (slicer_rays_observe(rh, rt->chis[s], rt_out) != SLICER_OK)
                return fail(h, "slicer_amd: --raytrace");
            for (int k = 0; k < SLICER_RAYS_COUNT; k++)
                if (slicer_copy_to_host(h, map.data(), rt_out[k], map.size() * sizeof(float)) != SLICER_OK ||
                    !save("ray-traced", token[k], zbuf, map, keys))
                    return fail(h, "slicer_amd: --raytrace");
        }
        return 0;
    }

    // The planes i0 .. i1-1 of one pass go into the kappa maps as ONE batch whether they were deposited now (their
    // finalized maps on the root, plane k of `todo`) or read back from the files a previous run left (resume): the
    // batches, and with them the roundings, are the same in both cases.
    int add_pass(int i0, int i1, const vector<int> &todo)
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
                const size_t slot = n_up++;
                void *b = nullptr;
                if (upload.size() <= slot) {
                    if (slicer_device_malloc(h, np2 * sizeof(float), &b) != SLICER_OK)
                        return fail(h, "slicer_amd");
                    upload.push_back((float *)b);
                }
                d = upload[slot];
                // (stream-ordered after the previous batch's kernels, which may still read this buffer)
                if (slicer_copy_to_device(h, d, host.data(), np2 * sizeof(float)) != SLICER_OK)
                    return fail(h, "slicer_amd");
            }
            maps.push_back(d);
            for (size_t s = 0; s < zs.size(); s++)
                c.push_back(coeff[s * lens.nplanes + i]);
        }
        if (slicer_kappa_add(kh, (int)maps.size(), maps.data(), c.data()) != SLICER_OK)
            return fail(h, "slicer_amd: --kappa");
        for (int i = i0; rt && i < i1; i++)
            if (const int rc = trace_plane(i, maps[i - i0]))
                return rc;
        return 0;
    }

    bool save(const char *what, const char *token, const char *zbuf, const vector<float> &map, const FitsKey *keys)
    {
        const string path = p.directory + p.simulation + token + zbuf + "_" + p.snpix + "_" + p.suffix + ".fits";
        cout << "Saving the " << what << " map on: " << path << endl;
        if (fits_write_image(path, map.data(), p.npix, keys, 2))
            return true;
        cerr << "It was not possible to create the map: " << path << endl;
        return false;
    }

    // One f32 FITS per source: the keys of kslicer's genericHeader (ZSOURCE, ANGLE).  With --shear, smr.smr(kappa file)
    // next to it: the same name with the .kappa_z token replaced, the same header.
    int write()
    {
        vector<float> map((size_t)p.npix * (size_t)p.npix);
        if (slicer_kappa_finalize(kh) != SLICER_OK)
            return fail(h, "slicer_amd: --kappa");
        struct Out {
            const char *what, *token;
            int which;
        };
        vector<Out> outs = {{"shear", ".gamma1_z", gradient ? SLICER_SHEAR_FD_GAMMA1 : SLICER_SHEAR_GAMMA1},
                            {"shear", ".gamma2_z", gradient ? SLICER_SHEAR_FD_GAMMA2 : SLICER_SHEAR_GAMMA2},
                            {"shear", ".gamma_z", gradient ? SLICER_SHEAR_FD_GAMMA : SLICER_SHEAR_GAMMA},
                            {"shear", ".phi_z", SLICER_SHEAR_PHI}};
        if (deflection) {
            outs.push_back({"deflection", ".alpha1_z", gradient ? SLICER_SHEAR_FD_ALPHA1 : SLICER_SHEAR_ALPHA1});
            outs.push_back({"deflection", ".alpha2_z", gradient ? SLICER_SHEAR_FD_ALPHA2 : SLICER_SHEAR_ALPHA2});
        }
        const int nlev = moments_levels + 1;  // (0 without --moments)
        vector<int32_t> mom_npix(nlev);
        vector<double> mom_mean(zs.size() * nlev), mom_sums(zs.size() * nlev * SLICER_MOMENTS_ORDERS);
        const int pk_lev = pkh ? std::max(nlev, 1) : 0;  // levels 0 ... L of the pyramid, level 0 alone without --moments
        const size_t pk_row = pkh ? 3 * (peaks_edges.size() - 1) + 7 : 0;
        vector<int64_t> pk_counts(zs.size() * pk_lev * pk_row);
        for (size_t s = 0; s < zs.size(); s++) {
            char zbuf[32];
            snprintf(zbuf, sizeof zbuf, "%.4f", zs[s]);
            const FitsKey keys[2] = {{"ZSOURCE", false, 0, zs[s], " "}, {"ANGLE", false, 0, p.fov, " "}};
            if (slicer_kappa_read(kh, (int)s, map.data()) != SLICER_OK || !save("convergence", ".kappa_z", zbuf, map, keys))
                return fail(h, "slicer_amd: --kappa");
            if (!shear_files && !mh && !pkh)
                continue;
            float *d_kappa = nullptr;
            if (slicer_kappa_device_map(kh, (int)s, &d_kappa) != SLICER_OK)
                return fail(h, "slicer_amd: --kappa");
            if (mh && (slicer_moments_run(mh, d_kappa, nullptr) != SLICER_OK ||
                       slicer_moments_read(mh, mom_npix.data(), &mom_mean[s * nlev], nullptr,
                                           &mom_sums[s * nlev * SLICER_MOMENTS_ORDERS]) != SLICER_OK))
                return fail(h, "slicer_amd: --moments");
            for (int l = 0; l < pk_lev; l++) {  // (after the moments: the pyramid's maps are those of this source)
                float *d_level = d_kappa;
                if (l > 0 && slicer_moments_device_map(mh, l, &d_level) != SLICER_OK)
                    return fail(h, "slicer_amd: --peaks");
                const size_t B = peaks_edges.size() - 1;
                int64_t *c = &pk_counts[(s * pk_lev + l) * pk_row];  // pdf, peaks, minima [B]; below, above [3]; nan
                if (slicer_peaks_run_npix(pkh, d_level, p.npix >> l) != SLICER_OK ||
                    slicer_peaks_read(pkh, c, c + B, c + 2 * B, c + 3 * B, c + 3 * B + 3, c + 3 * B + 6) != SLICER_OK)
                    return fail(h, "slicer_amd: --peaks");
            }
            if (!shear_files)
                continue;
            if (slicer_shear_run(shh, d_kappa) != SLICER_OK)
                return fail(h, "slicer_amd: --kappa");
            if ((gradient && slicer_shear_fd(shh) != SLICER_OK) ||
                (deflection && !gradient && slicer_shear_deflection(shh) != SLICER_OK))
                return fail(h, "slicer_amd: --shear");
            for (const auto &o : outs)
                if (slicer_shear_read(shh, o.which, map.data()) != SLICER_OK || !save(o.what, o.token, zbuf, map, keys))
                    return fail(h, "slicer_amd: --kappa");
        }
        if (const int rc = ph ? write_power() : 0)
            return rc;
        if (const int rc = mh ? write_moments(mom_npix, mom_mean, mom_sums) : 0)
            return rc;
        return pkh ? write_peaks(pk_lev, pk_counts) : 0;
    }

    // The histograms of the kappa maps, one text file: '#' lines (npix, angle, levels, the edges, column names), then per
    // (source, level) one row per bin: -1 (below the first edge), 0 ... B-1, B (above the last), B+1 (NaN pixels)
    int write_peaks(int nlev, const vector<int64_t> &counts)
    {
        const string path = p.directory + p.simulation + ".peaks_" + p.snpix + "_" + p.suffix + ".txt";
        cout << "Saving the histograms and peak counts on: " << path << endl;
        FILE *f = fopen(path.c_str(), "w");
        if (!f) {
            cerr << "It was not possible to create the file: " << path << endl;
            return 1;
        }
        const int B = (int)peaks_edges.size() - 1;
        const size_t row = 3 * (size_t)B + 7;
        fprintf(f, "# npix %d\n# angle_deg %.17g\n# levels %d\n# edges", p.npix, p.fov, nlev - 1);
        for (double e : peaks_edges)
            fprintf(f, " %.17g", e);
        fprintf(f, "\n# z level npix bin lo hi n_pixels n_peaks n_minima\n");
        for (size_t s = 0; s < zs.size(); s++)
            for (int l = 0; l < nlev; l++) {
                const int64_t *c = &counts[(s * nlev + l) * row];
                const int64_t *below = c + 3 * B, *above = below + 3;
                char head[96];
                snprintf(head, sizeof head, "%.17g %d %d", zs[s], l, p.npix >> l);
                fprintf(f, "%s -1 -inf %.17g %lld %lld %lld\n", head, peaks_edges[0], (long long)below[0],
                        (long long)below[1], (long long)below[2]);
                for (int b = 0; b < B; b++)
                    fprintf(f, "%s %d %.17g %.17g %lld %lld %lld\n", head, b, peaks_edges[b], peaks_edges[b + 1],
                            (long long)c[b], (long long)c[B + b], (long long)c[2 * B + b]);
                fprintf(f, "%s %d %.17g inf %lld %lld %lld\n", head, B, peaks_edges[B], (long long)above[0],
                        (long long)above[1], (long long)above[2]);
                fprintf(f, "%s %d nan nan %lld 0 0\n", head, B + 1, (long long)c[3 * B + 6]);
            }
        if (fclose(f) != 0) {
            cerr << "It was not possible to write the file: " << path << endl;
            return 1;
        }
        return 0;
    }

    // The moments of the kappa maps, one text file: '#' lines (npix, angle, levels, column names), then per (source,
    // level) z level npix mean S2 ... S8 (%.17g): the raw sums about the level's own mean
    int write_moments(const vector<int32_t> &npix_level, const vector<double> &mean, const vector<double> &sums)
    {
        const string path = p.directory + p.simulation + ".moments_" + p.snpix + "_" + p.suffix + ".txt";
        cout << "Saving the moments on: " << path << endl;
        FILE *f = fopen(path.c_str(), "w");
        if (!f) {
            cerr << "It was not possible to create the file: " << path << endl;
            return 1;
        }
        const int nlev = moments_levels + 1;
        fprintf(f, "# npix %d\n# angle_deg %.17g\n# levels %d\n# z level npix mean", p.npix, p.fov, moments_levels);
        for (int k = 2; k < 2 + SLICER_MOMENTS_ORDERS; k++)
            fprintf(f, " S%d", k);
        fprintf(f, "\n");
        for (size_t s = 0; s < zs.size(); s++)
            for (int l = 0; l < nlev; l++) {
                fprintf(f, "%.17g %d %d %.17g", zs[s], l, (int)npix_level[l], mean[s * nlev + l]);
                for (int k = 0; k < SLICER_MOMENTS_ORDERS; k++)
                    fprintf(f, " %.17g", sums[(s * nlev + l) * SLICER_MOMENTS_ORDERS + k]);
                fprintf(f, "\n");
            }
        if (fclose(f) != 0) {
            cerr << "It was not possible to write the file: " << path << endl;
            return 1;
        }
        return 0;
    }

    // The binned spectra of the kappa maps, one text file: '#' lines (npix, angle, source redshifts, column names),
    // then per bin ell_lo ell_hi ell_mean n_modes and C of every pair (%.17g; nan for an empty bin)
    int write_power()
    {
        const int S = (int)zs.size(), ne = power_edges.empty() ? p.npix : (int)power_edges.size(), B = ne - 1;
        const bool cross = power_mode == "cross";
        vector<const float *> maps(S);
        for (int s = 0; s < S; s++) {
            float *d = nullptr;
            if (slicer_kappa_device_map(kh, s, &d) != SLICER_OK)
                return fail(h, "slicer_amd: --power");
            maps[s] = d;
        }
        vector<std::pair<int, int>> pairs;
        for (int s = 0; s < S; s++)
            for (int t = s; t < (cross ? S : s + 1); t++)
                pairs.emplace_back(s, t);
        vector<double> cl(pairs.size() * B), ell(B);
        vector<int64_t> counts(B);
        if (slicer_power_run(ph, maps.data()) != SLICER_OK ||
            slicer_power_read(ph, cl.data(), ell.data(), counts.data()) != SLICER_OK)
            return fail(h, "slicer_amd: --power");
        const string path = p.directory + p.simulation + ".cl_" + p.snpix + "_" + p.suffix + ".txt";
        cout << "Saving the power spectra on: " << path << endl;
        FILE *f = fopen(path.c_str(), "w");
        if (!f) {
            cerr << "It was not possible to create the file: " << path << endl;
            return 1;
        }
        const double ell_f = 2.0 * M_PI / (p.fov * M_PI / 180.0);
        fprintf(f, "# npix %d\n# angle_deg %.17g\n# zs", p.npix, p.fov);
        for (double z : zs)
            fprintf(f, " %.17g", z);
        fprintf(f, "\n# ell_lo ell_hi ell_mean n_modes");
        for (const auto &pr : pairs)
            fprintf(f, " C_%d_%d", pr.first, pr.second);
        fprintf(f, "\n");
        for (int b = 0; b < B; b++) {
            const double lo = power_edges.empty() ? (double)b : power_edges[b];
            const double hi = power_edges.empty() ? (double)(b + 1) : power_edges[b + 1];
            fprintf(f, "%.17g %.17g %.17g %lld", lo * ell_f, hi * ell_f, ell[b], (long long)counts[b]);
            for (size_t q = 0; q < pairs.size(); q++)
                fprintf(f, " %.17g", cl[q * B + b]);
            fprintf(f, "\n");
        }
        if (fclose(f) != 0) {
            cerr << "It was not possible to write the file: " << path << endl;
            return 1;
        }
        return 0;
    }
};

// The root's maps of the planes `todo` of a finished pass, into their files (slicer-v2.cpp:219-226)
int write_planes(const Options &o, Cone &c, slicer_handle h, const vector<int> &todo, const Header &simhdr)
{
    InputParams &p = c.p;
    const size_t np2 = (size_t)p.npix * (size_t)p.npix;
    std::valarray<float> tot(np2), toti[6];
    for (size_t k = 0; k < todo.size(); k++) {
        const int i = todo[k];
        int64_t nsel[6];
        float *d_toti[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (slicer_plane_read(h, (int)k, &tot[0], nullptr, nsel) != SLICER_OK ||
            (p.partinplanes && slicer_plane_device_maps(h, (int)k, nullptr, d_toti) != SLICER_OK))
            return fail(h, "slicer_amd");
        int ntotxyi[6];
        for (int t = 0; t < 6; t++) {
            ntotxyi[t] = o.reference_counts ? 0 : (int)nsel[t];
            if (!p.partinplanes)
                continue;
            // per-type maps straight from the device into the array writeMaps gets; types without particles: zeros
            if (toti[t].size() != np2)
                toti[t].resize(np2);
            if (!d_toti[t])
                toti[t] = 0.0f;
            else if (slicer_copy_to_host(h, &toti[t][0], d_toti[t], np2 * sizeof(float)) != SLICER_OK)
                return fail(h, "slicer_amd");
        }
        const double zsim = c.getZl.eval((c.lens.ld2[i] + c.lens.ld[i]) / 2.0);  // slicer-v2.cpp:219
        Header hd = simhdr;
        try {
            writeMaps(p, hd, c.lens, i, zsim, plane_label(c.lens.pll[i]), p.snpix, tot, toti, ntotxyi, myid);
        } catch (const std::runtime_error &) {
            return 1;
        }
    }
    return 0;
}

// One pass that has planes to make: every rank deposits its share of the sub-files, the rank sum onto the root, the
// root writes the planes
int make_planes(const Options &o, Cone &c, Ranks &ranks, int isnap, float rcase, const vector<int> &todo)
{
    const string File = c.p.pathsnap + c.lens.fromsnap[isnap];
    Header simhdr;
    if (!read_header(File, simhdr))
        return 1;
    const slicer_plane_desc d = plane_desc(c.p, c.lens, todo, o.mas, o.accum, SLICER_ALGO_AUTO,
                                           c.p.partinplanes ? 1 : 0, c.fovradiants);
    const int algo = o.reduce_algo == "direct" ? SLICER_RCCL_REDUCE_DIRECT : SLICER_RCCL_REDUCE_ROOTED;
    const int n = (int)ranks.r.size();
    vector<int> rc(n, 0);
    Rendezvous rendezvous(n);
    // one rank's share of the pass: its contiguous range of sub-files (slicer-v2.cpp:162-175: numfiles / nranks each,
    // the last rank takes the remainder), then the rank sum
    auto run_rank = [&](int k) {
        const Rank &R = ranks.r[k];
        const string who = "slicer_amd (device " + std::to_string(R.device) + ")";
        if (slicer_plane_begin(R.h, &d) != SLICER_OK)
            rc[k] = fail(R.h, who + ": plane_begin");
        const int per = simhdr.numfiles / n, ffmax = k == n - 1 ? simhdr.numfiles : (k + 1) * per;
        for (int ff = k * per; ff < ffmax && rc[k] == 0; ff++)
            rc[k] = deposit_subfile(R.h, File + "." + std::to_string(ff), c.p.hydro, c.random, isnap, rcase, who);
        // slicer-v2.cpp:214-217: the sum over ranks onto the root, here over RCCL on the accumulators.  The ranks
        // agree on the outcome of the deposit phase first: the collective is entered by all of them or by none.
        if (n > 1 && rendezvous.any_failed(rc[k] != 0)) {
            if (rc[k] == 0)
                cerr << who << ": another rank failed; skipping the rank sum" << endl;
            rc[k] = 1;
        } else if (R.comm && ranks.rccl.plane_reduce(R.h, R.comm, 0, algo) != SLICER_OK) {
            cerr << who << ": rank sum: " << ranks.rccl.last_error() << endl;
            rc[k] = 1;
        }
    };
    vector<std::thread> threads;
    for (int k = 1; k < n; k++)
        threads.emplace_back(run_rank, k);
    run_rank(0);
    for (auto &t : threads)
        t.join();
    if (std::count(rc.begin(), rc.end(), 0) != n ||
        (n > 1 && o.reduce_mode == "host" && host_plane_reduce(ranks.r, c.p.npix, (int)todo.size())))
        return 1;
    return write_planes(o, c, ranks.root(), todo, simhdr);
}

// The plane loop (slicer-v2.cpp:137-229)
int run_planes(const Options &o, Cone &c, Ranks &ranks, LensingOutputs &lensing)
{
    InputParams &p = c.p;
    const Lens &lens = c.lens;
    cout << " Now loop on " << lens.nplanes << " planes " << endl;
    float rcase = 0.0f;  // slicer-v2.cpp:137
    for (int isnap = 0, iend; isnap < lens.nplanes; isnap = iend) {
        // planes isnap .. iend-1 share snapshot, Random entry and rcase: one pass.  (snopt > 0: thinning consumes libc
        // rand() plane by plane, densitymaps.cpp:387-397.  A pass over several planes keeps that order -- the library
        // replays its chunks plane-major when the pass ends -- so the planes of a box replication still share one read
        // of the snapshot.)
        iend = isnap + 1;
        if (!o.single_plane && !p.physical)
            while (iend < lens.nplanes && iend - isnap < SLICER_MAX_PLANES && !lens.randomize[iend] &&
                   lens.fromsnapi[iend] == lens.fromsnapi[isnap] && lens.nrepperp[iend] == lens.nrepperp[isnap])
                iend++;
        if (p.physical)  // slicer-v2.cpp:142-143
            p.npix = int((lens.ld2[isnap] + lens.ld[isnap]) / 2 * c.fovradiants / p.rgrid * 1e3 / kPosU) + 1;
        if (lens.randomize[isnap])  // slicer-v2.cpp:184-185
            rcase = (float)(lens.ld[isnap] / c.snapbox[lens.fromsnapi[isnap]] * 1e3 / kPosU);
        // resume: planes whose output exists are skipped (slicer-v2.cpp:188-202, only when !partinplanes)
        vector<int> todo;
        for (int i = isnap; i < iend; i++) {
            const string path = fileOutput(p, plane_label(lens.pll[i]));
            if (!p.partinplanes && file_exists(path))
                cout << path << " Already exists" << endl;
            else
                todo.push_back(i);
        }
        if (p.partinplanes && isnap == 0)
            cout << "!It is not possible to resume a Gadget run with partinplanes == true!" << endl;
        if ((!todo.empty() && make_planes(o, c, ranks, isnap, rcase, todo)) ||
            (lensing.kh && lensing.add_pass(isnap, iend, todo)))
            return 1;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Options o;
    if (const int rc = parse_args(argc, argv, o))
        return rc;
    Cone c;
    if (const int rc = plan_cone(o, c))
        return rc;
    if (o.plan_only)
        return 0;
    vector<double> kappa_zs, kappa_c;
    if (const int rc = kappa_weights(o, c, kappa_zs, kappa_c))
        return rc;
    RayPlan ray_plan;
    if (const int rc = raytrace_plan(o, c, kappa_zs, ray_plan))
        return rc;
    const vector<int> devs = o.devices_spec.empty() ? vector<int>{o.device} : parse_devices(o.devices_spec);
    if (devs.empty() || (o.reduce_mode != "rccl" && o.reduce_mode != "host") ||
        (o.reduce_algo != "rooted" && o.reduce_algo != "direct")) {
        cerr << "bad --devices / --reduce / --reduce-algo" << endl;
        return 2;
    }
    Ranks ranks;
    if (const int rc = ranks.create(devs, c.p.snopt, o.reduce_mode == "rccl"))
        return rc;
    LensingOutputs lensing{ranks.root(), c.p, c.lens, kappa_zs, kappa_c};  // (after `ranks`, see there)
    lensing.deflection = o.deflection;
    lensing.gradient = o.shear_derivative == "gradient";
    lensing.power_mode = o.power;
    lensing.power_edges = o.power_edges;
    lensing.moments_levels = o.moments ? o.moments_levels : -1;
    lensing.peaks_edges = o.peaks_edges;
    lensing.rt = o.raytrace ? &ray_plan : nullptr;
    if (const int rc = lensing.create(o.shear))
        return rc;
    const int rc = run_planes(o, c, ranks, lensing);
    return rc == 0 && lensing.kh ? lensing.write() : rc;
}
