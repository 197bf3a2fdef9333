"""Times slicer_minkowski_run (the counting kernel and its finish kernels) at 4096^2 and 16384^2 on a white-noise map
with T = 9, 65 and 1025 uniform thresholds between -4 and +4 sigma, and once with every pixel at one rank (T = 65 with
thresholds far outside the map's range but the first: every lane of a wave increments the same LDS counters, the
contention case): 3 warm-up runs, then 20 timed runs, wall time over a stream synchronisation, and next to it the
kernel times of slicer_profile_* from a second set of 20 runs.  Prints the ratio to the HBM byte floor (computed at
6.3 TB/s, not measured): the map is read once, 4 B a pixel, and next to every case
slicer_peaks_run on the same map with the same T values as its B + 1 edges (B = T - 1), measured in the same session:
the two kernels share the search; this one makes five increments a cell against one to three.  Reported, not gated.
One JSON line per size."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402


def kernel_ms(s, call, reps, names):
    """Mean milliseconds a run of the kernels `names`, from the per-kernel profile of `reps` runs."""
    s.synchronize()
    s.profile_reset()
    s.profile_enable(True)
    for _ in range(reps):
        call()
    s.synchronize()
    prof = s.profile_get()
    s.profile_enable(False)
    return {k: round(prof[k][1] / prof[k][0], 4) for k in names if k in prof}


def main(sizes=(4096, 16384), reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            d = s.to_device(rng.standard_normal((n, n), np.float32))
            out = {"npix": n}
            cases = {f"T_{T}": slicer_amd.peaks_edges(-4.0, 4.0, T - 1) for T in (9, 65, 1025)}
            cases["one_rank_of_65"] = slicer_amd.peaks_edges(-50.0, 6350.0, 64)  # rank 1 is -50 ... 50: every pixel
            try:
                for name, t in cases.items():
                    with slicer_amd.Minkowski(s, n, t) as m:
                        dt = timed(s, lambda: m.run(d), reps)
                        r = m.read()
                        kernels = kernel_ms(s, lambda: m.run(d), reps, ("minkowski", "minkowski_finish"))
                    assert r["faces"][0] <= n * n and r["euler"][0] == r["vertices"][0] - r["edges"][0] + r["faces"][0]
                    out[name] = report(4 * n * n, dt)
                    out[name]["kernel_ms"] = kernels
                    out[name]["faces_fraction_first_last"] = [round(float(r["faces"][k]) / (n * n), 4) for k in (0, -1)]
                    with slicer_amd.Peaks(s, n, t) as p:
                        dp = timed(s, lambda: p.run(d), reps)
                        p.read()
                        kernels = kernel_ms(s, lambda: p.run(d), reps, ("peaks", "peaks_finish"))
                    out[name]["peaks_same_edges"] = {"ms_per_run": round(dp * 1e3, 3), "kernel_ms": kernels,
                                                     "minkowski_over_peaks": round(dt / dp, 2)}
            finally:
                s.free(d)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
