// subfile_deposit.hpp -- what the createDensityMaps adapter and the SLICER_amd driver share above the C ABI.
#pragma once
#include <string>
#include <vector>

#include "../../include/slicer_amd.h"
#include "slicer_types.hpp"

namespace slicer_amd {

// "<who>: <slicer_last_error(h)>" on std::cerr (h may be NULL); returns 1
int fail(slicer_handle h, const std::string &who);

// a sub-file's header fields and the Random entry isnap of its plane, as the deposit reads them
slicer_file_desc file_desc(const Header &data, const Random &random, int isnap, float rcase);

// one pass over the lens planes `planes` (at most SLICER_MAX_PLANES) of one box replication
slicer_plane_desc plane_desc(const InputParams &p, const Lens &lens, const std::vector<int> &planes, int mas, int accum,
                             int algo, int want_type_maps, double fov_rad);

// Sub-file `path` into the pass open on h: POS (with hydro, the MASS / BHMA masses), with Random entry isnap and rcase.
// 0, or 1 after a message on std::cerr (prefixed with `who`, except the reference's "Error in opening the file").
// Keeps no state between calls: rank threads call it at the same time, each on its own handle.
int deposit_subfile(slicer_handle h, const std::string &path, int hydro, const Random &random, int isnap, float rcase,
                    const std::string &who);

}  // namespace slicer_amd
