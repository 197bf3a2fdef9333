"""Times the E/B pseudo-C_l handle next to the scalar one (row N17) in the same process, on
4096^2 white-noise maps with a 64-pixel border taper and 32 log bins, tools/pcl_bench.py's case: slicer_pcl2_set_mask
(the mask, its moments, the autocorrelation and per bin one column of M0, M2, X2, M4 and X4: five band inverses and five
forward transforms against slicer_pcl_set_mask's one and one; both wait for the stream themselves) and slicer_pcl2_run
of one field (gamma1, gamma2, kappa) next to slicer_pcl_run of the same three maps in cross mode; 2 warm-up runs, then 5
timed ones of set_mask and 20 of run, wall time over a stream synchronisation.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402

N, TAPER_PIX, BINS, WARM, MASK_REPS, RUN_REPS, ANGLE = 4096, 64.0, 32, 2, 5, 20, 10.0


def timed(s, call, reps):
    for _ in range(WARM):
        call()
    s.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    s.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    edges = np.concatenate([[0.0], np.geomspace(1.0, 0.75 * N, BINS)])
    rng = np.random.default_rng(N)
    with slicer_amd.Slicer(0) as s:
        d = [s.to_device(rng.standard_normal((N, N)).astype(np.float32)) for _ in range(3)]
        try:
            active = int((slicer_amd.power_bins(N, edges)["counts"] > 0).sum())
            with slicer_amd.Pcl(s, N, ANGLE, 3, cross=True, edges=edges) as p:
                pcl_mask_ms = timed(s, lambda: p.set_mask(None, TAPER_PIX), MASK_REPS)
                pcl_run_ms = timed(s, lambda: p.run(d), RUN_REPS)
            with slicer_amd.PclShear(s, N, ANGLE, 1, with_kappa=True, cross=True, edges=edges) as q:
                eb_mask_ms = timed(s, lambda: q.set_mask(None, TAPER_PIX), MASK_REPS)
                eb_run_ms = timed(s, lambda: q.run(d), RUN_REPS)
        finally:
            for x in d:
                s.free(x)
    print(json.dumps({"npix": N, "taper_pix": TAPER_PIX, "bins": BINS, "active_bins": active,
                      "pcl_shear_set_mask_ms": round(eb_mask_ms, 3), "pcl_set_mask_ms": round(pcl_mask_ms, 3),
                      "set_mask_ratio": round(eb_mask_ms / pcl_mask_ms, 3),
                      "pcl_shear_run_ms": round(eb_run_ms, 3), "pcl_run_ms": round(pcl_run_ms, 3),
                      "run_ratio": round(eb_run_ms / pcl_run_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
