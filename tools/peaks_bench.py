"""Times slicer_peaks_run (the histogram kernel and its finish kernel) at 4096^2 and 16384^2 on a white-noise map with
B = 64 and B = 1024 uniform bins between -5 and +5 sigma, and once with every pixel in a single bin (B = 64 with edges
far outside the map's range: every lane of a wave increments one LDS counter, the contention case): 3 warm-up runs,
then 20 timed runs, wall time over a stream synchronisation.  Prints the ratio to the HBM byte floor (computed at
6.3 TB/s, not measured): the map is read once, 4 B a pixel.  The project's goal is 3x the floor;
it is reported here, not gated.  One JSON line per size."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402


def main(sizes=(4096, 16384), reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            d = s.to_device(rng.standard_normal((n, n), np.float32))
            out = {"npix": n}
            cases = {"bins_64": slicer_amd.peaks_edges(-5.0, 5.0, 64), "bins_1024": slicer_amd.peaks_edges(-5.0, 5.0, 1024),
                     "one_bin_of_64": slicer_amd.peaks_edges(-50.0, 6350.0, 64)}  # bin 0 is -50 ... 50: every pixel
            try:
                for name, edges in cases.items():
                    with slicer_amd.Peaks(s, n, edges) as p:
                        dt = timed(s, lambda: p.run(d), reps)
                        r = p.read()
                    assert int(r["pdf"].sum() + r["below"][0] + r["above"][0] + r["nan"]) == n * n
                    out[name] = report(4 * n * n, dt)
                    out[name]["largest_bin_fraction"] = round(float(r["pdf"].max()) / (n * n), 4)
            finally:
                s.free(d)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
