"""Times the masked pseudo-C_l handle on a 4096^2 white-noise map with a 64-pixel border taper
and 32 log bins: slicer_pcl_set_mask (the mask, its moments, the autocorrelation and one column of the coupling matrix
per bin; it waits for the stream itself) in total and per bin, and slicer_pcl_run next to slicer_power_run on the same
map in the same process; 3 warm-up runs, then 20 timed ones, wall time over a stream synchronisation.  A column of the
matrix is one band inverse, one forward transform and one binning: the floor it is set against is the sum of what the
same process measures for those three through slicer_profile_* (the band inverse of a Bispectrum handle on the same
bins, the forward transform and the binning of the Power handle).  One JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402

N, TAPER_PIX, BINS, WARM, REPS, ANGLE = 4096, 64.0, 32, 3, 20, 10.0


def timed(s, call, reps=REPS):
    for _ in range(WARM):
        call()
    s.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    s.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def profiled(s, call, names, reps=REPS):
    s.profile_enable(True)
    s.profile_reset()
    for _ in range(reps):
        call()
    s.synchronize()
    prof = s.profile_get()
    s.profile_enable(False)
    return [prof[k][1] / prof[k][0] for k in names]  # ms per launch group


def main():
    edges = np.concatenate([[0.0], np.geomspace(1.0, 0.75 * N, BINS)])
    rng = np.random.default_rng(N)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((N, N)).astype(np.float32))
        try:
            with slicer_amd.Pcl(s, N, ANGLE, 1, edges=edges) as p:
                active = int((slicer_amd.power_bins(N, edges)["counts"] > 0).sum())
                set_mask_ms = timed(s, lambda: p.set_mask(None, TAPER_PIX))
                run_ms = timed(s, lambda: p.run([d]))
            with slicer_amd.Power(s, N, ANGLE, 1, edges=edges) as pw:
                power_ms = timed(s, lambda: pw.run([d]))
                forward_ms, binning_ms = profiled(s, lambda: pw.run([d]), ("power_fft", "power_bin"))
            with slicer_amd.Bispectrum(s, N, ANGLE, edges=edges, triples="equilateral") as b:
                b.run(d)
                (bands_ms,) = profiled(s, lambda: b.run(d), ("bispectrum_band",), reps=3)
                band_ms = bands_ms / BINS  # one scope times the inverses of all the bins, empty ones included
        finally:
            s.free(d)
    floor = band_ms + forward_ms + binning_ms
    per_bin = set_mask_ms / active
    print(json.dumps({"npix": N, "taper_pix": TAPER_PIX, "bins": BINS, "active_bins": active,
                      "set_mask_ms": round(set_mask_ms, 3), "set_mask_ms_per_bin": round(per_bin, 3),
                      "band_inverse_ms": round(band_ms, 3), "forward_ms": round(forward_ms, 3),
                      "binning_ms": round(binning_ms, 3), "per_bin_floor_ms": round(floor, 3),
                      "per_bin_over_floor": round(per_bin / floor, 3),
                      "pcl_run_ms": round(run_ms, 3), "power_run_ms": round(power_ms, 3),
                      "pcl_run_over_power_run": round(run_ms / power_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
