"""Times slicer_power_run (forward r2c transforms + binning) at 4096^2 with 1 map (auto) and 8 maps (cross), and at
16384^2 with 1 map: 3 warm-up runs, then 20 timed runs.  The forward transforms and the binning are timed apart through
slicer_profile_* (HIP events around each); the wall time of a run is taken over a stream synchronisation.  Each is
reported against its byte floor at the HBM peak: the forward passes move the bytes tools/shear_bench.py counts for the
forward half, and the binning reads every spectrum once (16 n (n/2+1) bytes per map).  One JSON line per case."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shear_bench  # noqa: E402
import slicer_amd  # noqa: E402

HBM_BYTES_PER_S = shear_bench.HBM_BYTES_PER_S  # MI355X peak HBM bandwidth (computed floor, not measured)


def forward_bytes(n):
    H, even = n // 2 + 1, n % 2 == 0
    row_c = 16 * (n * (n // 2) if even else (n + 1) // 2 * n)
    col_c = 16 * n * H
    mr = shear_bench.passes(n // 2 if even else n, shear_bench.LDS_POINTS)
    mc = shear_bench.passes(n, shear_bench.COL_CAP)
    return 4 * n * n + row_c + 2 * row_c * (mr - 1) + row_c + col_c + 2 * col_c * (mc - 1)


def case(s, n, S, cross, reps=20, angle=10.0):
    rng = np.random.default_rng(n + S)
    ptrs = [s.to_device(rng.standard_normal((n, n)).astype(np.float32)) for _ in range(S)]
    try:
        with slicer_amd.Power(s, n, angle, S, cross=cross) as p:
            for _ in range(3):
                p.run(ptrs)
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                p.run(ptrs)
            s.synchronize()
            wall = (time.perf_counter() - t0) / reps
            s.profile_enable(True)
            s.profile_reset()
            for _ in range(reps):
                p.run(ptrs)
            s.synchronize()
            prof = s.profile_get()
            s.profile_enable(False)
    finally:
        for d in ptrs:
            s.free(d)
    fft_ms = prof["power_fft"][1] / reps
    bin_ms = prof["power_bin"][1] / reps
    fb, bb = S * forward_bytes(n), S * 16 * n * (n // 2 + 1)
    fft_floor, bin_floor = fb / HBM_BYTES_PER_S * 1e3, bb / HBM_BYTES_PER_S * 1e3
    return {"npix": n, "maps": S, "mode": "cross" if cross else "auto", "ms_per_run": round(wall * 1e3, 3),
            "forward_ms": round(fft_ms, 3), "forward_floor_ms": round(fft_floor, 3),
            "forward_fraction_of_floor": round(fft_floor / fft_ms, 3),
            "binning_ms": round(bin_ms, 3), "binning_floor_ms": round(bin_floor, 3),
            "binning_fraction_of_floor": round(bin_floor / bin_ms, 3)}


def main():
    with slicer_amd.Slicer(0) as s:
        for n, S, cross in ((4096, 1, False), (4096, 8, True), (16384, 1, False)):
            print(json.dumps(case(s, n, S, cross)), flush=True)


if __name__ == "__main__":
    main()
