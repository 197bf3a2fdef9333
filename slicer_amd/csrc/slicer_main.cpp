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
//   * --kappa with --shear, --deflection, --shear-derivative, --raytrace, --power, --pcl, --pcl-shear, --xi, --moments, --peaks, --minkowski, --betti, --bispectrum, --smooth, --shape-noise, --starlet, --scattering and --catalogue adds the
//     lensing outputs computed on device 0 from the finalized planes (driver_lensing.cpp describes them)
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
#include "driver_lensing.hpp"
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
    string inifile, plan_path, devices_spec, reduce_mode = "rccl", reduce_algo = "rooted";
    LensingOptions lensing;
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
        else if (const int rc = o.lensing.parse(argc, argv, i); rc >= 0) {
            if (rc)
                return rc;
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
    return o.lensing.check();
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
    if (const int rc = o.lensing.check_npix(p))  // on the host, before any device work
        return rc;
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
    LensingPlan plan;  // (host only: before any device is opened)
    if (const int rc = plan_lensing(o.lensing, c.p, c.simdata, c.lens, plan))
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
    LensingOutputs lensing{ranks.root(), o.lensing, plan, c.p, c.lens};  // (after `ranks`: released before them)
    if (const int rc = lensing.create())
        return rc;
    const int rc = run_planes(o, c, ranks, lensing);
    return rc == 0 && lensing.kh ? lensing.write() : rc;
}
