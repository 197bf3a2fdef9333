"""Times PeakCatalogue.run (count, scan, emit: slicer_catalogue_run) next to Peaks.run (slicer_peaks_run, B = 64) on the
same 4096^2 white-noise map in the same process, peaks only: with min_peak = -inf, which keeps every peak (about a
ninth of the interior), and with the threshold that keeps about 1 % of them (the 99th percentile of the peaks'
heights): 3 warm-up runs, then 20 timed runs, wall time over a stream synchronisation.  Prints the ratio to the HBM byte
floor (computed at 6.3 TB/s, not measured): the map read twice (8 B a pixel), 32 B per stored record, and the segment
counts written by the count, read and rewritten by the scan and read by the emit (4 x 4 B per 64 pixels of a row)
(DESIGN.md S8 row N22).  The figures are reported, not gated.  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402


def main(n=4096, reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((n, n), np.float32))
        out = {"npix": n}
        try:
            with slicer_amd.Peaks(s, n, slicer_amd.peaks_edges(-5.0, 5.0, 64)) as p:
                out["peaks_bins_64"] = report(4 * n * n, timed(s, lambda: p.run(d), reps))
                r = p.read()
            n_peaks = int(r["peaks"].sum() + r["below"][1] + r["above"][1])
            segments = n * ((n + 63) // 64)
            with slicer_amd.PeakCatalogue(s, n, n * n // 4) as c:
                c.run(d)
                heights = c.read()["value"]
                assert len(heights) == n_peaks
                for name, min_peak in (("all_peaks", -np.inf), ("one_percent", float(np.percentile(heights, 99.0)))):
                    dt = timed(s, lambda: c.run(d, min_peak=min_peak), reps)
                    stored = c.counts()["stored"]
                    out[name] = report(8 * n * n + 32 * stored + 16 * segments, dt)
                    out[name]["records"] = stored
                    out[name]["times_peaks_run"] = round(dt * 1e3 / out["peaks_bins_64"]["ms_per_run"], 2)
        finally:
            s.free(d)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
