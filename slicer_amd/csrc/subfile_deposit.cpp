#include "subfile_deposit.hpp"

#include <algorithm>
#include <iostream>

#include "gadget2_reader.hpp"

namespace slicer_amd {

namespace {

// The POS block is streamed straight into the library's pinned staging buffers (no pageable copy of the block): file
// reads overlap with the H2D copies and kernels of the previous chunk.
struct Span {
    SnapshotFile *snap;
    long base;          // file offset of this type's first particle
    const float *mass;  // or nullptr
};

int fill(void *user, float *dst_pos, float *dst_mass, uint64_t first, uint64_t count)
{
    Span *s = static_cast<Span *>(user);
    if (!s->snap->read_at(s->base + (long)(12 * first), dst_pos, (size_t)(12 * count)))
        return 1;
    if (dst_mass)
        std::copy(s->mass + first, s->mass + first + count, dst_mass);
    return 0;
}

}  // namespace

int fail(slicer_handle h, const std::string &who)
{
    std::cerr << who << ": " << slicer_last_error(h) << std::endl;
    return 1;
}

slicer_file_desc file_desc(const Header &data, const Random &random, int isnap, float rcase)
{
    slicer_file_desc f{};
    for (int t = 0; t < 6; t++) {
        f.npart[t] = data.npart[t];
        f.massarr[t] = data.massarr[t];
    }
    f.boxsize = data.boxsize;
    f.sgn[0] = random.sgnX[isnap];
    f.sgn[1] = random.sgnY[isnap];
    f.sgn[2] = random.sgnZ[isnap];
    f.face = random.face[isnap];
    f.center[0] = random.x0[isnap];
    f.center[1] = random.y0[isnap];
    f.center[2] = random.z0[isnap];
    f.rcase = rcase;
    return f;
}

slicer_plane_desc plane_desc(const InputParams &p, const Lens &lens, const std::vector<int> &planes, int mas, int accum,
                             int algo, int want_type_maps, double fov_rad)
{
    slicer_plane_desc d{};
    d.npix = p.npix;
    d.n_planes = (int)planes.size();
    d.mas = mas;
    d.accum = accum;
    d.algo = algo;
    d.hydro = p.hydro ? 1 : 0;
    d.snopt = p.snopt;
    d.want_type_maps = want_type_maps;
    d.fov_rad = fov_rad;
    for (size_t k = 0; k < planes.size(); k++) {
        d.ld[k] = lens.ld[planes[k]];
        d.ld2[k] = lens.ld2[planes[k]];
        d.nrepperp[k] = lens.nrepperp[planes[k]];
    }
    return d;
}

int deposit_subfile(slicer_handle h, const std::string &path, int hydro, const Random &random, int isnap, float rcase,
                    const std::string &who)
{
    SnapshotFile snap;
    if (!snap.open(path)) {
        std::cerr << "Error in opening the file: " << path << "!\n\a";  // gadget2io.cpp:20
        return 1;
    }
    auto refuse = [&](const char *why) {
        std::cerr << who << ": " << snap.path() << ": " << why << std::endl;
        return 1;
    };
    const Header &data = snap.header();
    long pos_off = 0, pos_bytes = 0;
    if (!snap.locate_block("POS ", pos_off, pos_bytes))
        return refuse("no POS block");
    std::vector<float> mass[6];
    if (hydro && !snap.read_masses(mass))
        return refuse("cannot read MASS/BHMA");
    size_t ntot = 0;
    for (int t = 0; t < 6; t++)
        ntot += data.npart[t] > 0 ? (size_t)data.npart[t] : 0;
    // (the reads below stay inside the block: a header that claims more particles would deposit the next block)
    if (pos_bytes < 0 || (size_t)pos_bytes < 12 * ntot)
        return refuse("POS block shorter than the header says");
    const slicer_file_desc f = file_desc(data, random, isnap, rcase);
    if (slicer_file_begin(h, &f) != SLICER_OK)
        return fail(h, who + ": file_begin");
    size_t off = 0;
    for (int t = 0; t < 6; t++) {
        const size_t n = data.npart[t] > 0 ? (size_t)data.npart[t] : 0;
        if (n) {
            const float *m = (hydro && data.massarr[t] == 0 && !mass[t].empty()) ? mass[t].data() : nullptr;
            Span span{&snap, pos_off + (long)(12 * off), m};
            if (slicer_deposit_stream(h, t, n, m != nullptr, fill, &span) != SLICER_OK)
                return fail(h, who + ": deposit");
        }
        off += n;
    }
    if (slicer_file_end(h) != SLICER_OK)
        return fail(h, who + ": file_end");
    return 0;
}

}  // namespace slicer_amd
