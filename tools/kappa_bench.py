"""Times slicer_kappa_add at 4096^2: 4 device maps x {1, 8} sources, against the byte floor of one pass (every map
read once, every accumulator read and written once: (4 * 4 + S * 16) B per pixel).  Prints one JSON line per case."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # MI355X peak HBM bandwidth (computed floor, not measured)


def main(npix=4096, n_maps=4, reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(rng.random((npix, npix), dtype=np.float32)) for _ in range(n_maps)]
        for S in (1, 8):
            coeff = rng.uniform(1e-4, 1e-3, (n_maps, S))
            with slicer_amd.Kappa(s, npix, S) as k:
                for _ in range(3):
                    k.add_device(ptrs, coeff)
                s.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    k.add_device(ptrs, coeff)
                s.synchronize()
                dt = (time.perf_counter() - t0) / reps
            nbytes = npix * npix * (4 * n_maps + 16 * S)
            print(json.dumps({"npix": npix, "maps": n_maps, "sources": S, "ms_per_add": round(dt * 1e3, 4),
                              "bytes": nbytes, "GB_per_s": round(nbytes / dt / 1e9, 1),
                              "floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4),
                              "fraction_of_floor": round(nbytes / HBM_BYTES_PER_S / dt, 3)}))
        for p in ptrs:
            s.free(p)


if __name__ == "__main__":
    main()
