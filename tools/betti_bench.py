"""Times slicer_betti_run at 4096^2 and 16384^2 with T = 9, 65 and 1025 uniform thresholds between -4 and +4 sigma, on a
white-noise map (the worst case for the number of components) and on the same map smoothed with a Gaussian of 4 pixels
(the usual case): 3 warm-up runs, then `reps` timed runs, wall time over a stream synchronisation, and next to it the
kernel times of slicer_profile_* from a second set of runs (betti_rank: the ranks and their column sums; betti_link:
both sweeps, 2 T launches and the parents' reset; betti_finish), per run.  Prints the ratio to the HBM byte floor
(computed at 6.3 TB/s, not measured): the map read once (4 B a pixel), the u16 rank map written once and read by every
one of the 2 T link launches (2 n^2 T bytes a sweep), the parents written twice (4 n^2 each); what the unions
themselves move is not in the floor.  Next to every case slicer_minkowski_run of the same map and thresholds, measured
in the same session.  Reported, not gated.  One JSON line per size and map."""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402
from minkowski_bench import kernel_ms  # noqa: E402

SIGMA_PIX = 4.0


def floor_bytes(n, T):
    return 4 * n * n + 2 * n * n + 2 * (2 * n * n * T) + 2 * 4 * n * n


def main(sizes=(4096, 16384), reps=None):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            r_n = reps or (10 if n <= 4096 else 3)
            d = s.to_device(rng.standard_normal((n, n), np.float32))
            try:
                with slicer_amd.Smooth(s, n, "gauss", SIGMA_PIX) as sm:
                    sm.run(d)
                    # (the rms of unit white noise under a Gaussian of sigma pixels)
                    maps = {"white": (d, 1.0), "smoothed": (sm.device_map(), 1.0 / (2.0 * math.sqrt(math.pi) * SIGMA_PIX))}
                    for kind, (d_map, sigma) in maps.items():
                        out = {"npix": n, "map": kind, "reps": r_n}
                        for T in (9, 65, 1025):
                            t = slicer_amd.peaks_edges(-4.0 * sigma, 4.0 * sigma, T - 1)
                            with slicer_amd.Betti(s, n, t) as b:
                                dt = timed(s, lambda: b.run(d_map), r_n)
                                r = b.read()
                                kernels = kernel_ms(s, lambda: b.run(d_map), r_n, ("betti_rank", "betti_link", "betti_finish"))
                            with slicer_amd.Minkowski(s, n, t) as m:
                                dm = timed(s, lambda: m.run(d_map), r_n)
                                e = m.read()
                            assert np.array_equal(r["components"] - r["holes"], e["euler"])
                            c = out[f"T_{T}"] = report(floor_bytes(n, T), dt)
                            # (kernel_ms gives the mean per profiled scope: two betti_link scopes a run)
                            kernels["betti_link"] = round(2 * kernels["betti_link"], 4)
                            c["kernel_ms"] = kernels
                            c["components_first_max_last"] = [int(r["components"][0]), int(r["components"].max()),
                                                              int(r["components"][-1])]
                            c["holes_first_max_last"] = [int(r["holes"][0]), int(r["holes"].max()), int(r["holes"][-1])]
                            c["minkowski_ms_per_run"] = round(dm * 1e3, 3)
                            c["betti_over_minkowski"] = round(dt / dm, 1)
                        print(json.dumps(out), flush=True)
            finally:
                s.free(d)


if __name__ == "__main__":
    main()
