"""Times slicer_shear_deflection (two filtered inverse transforms of the kept spectrum) and slicer_fd_derivatives with
all six outputs at 4096^2 and 16384^2: 3 warm-up runs, then 20 timed runs, wall time over a stream synchronisation.
Prints the bytes each moves and the fraction of the HBM byte floor (computed at 6.3 TB/s, not measured): the stencil
kernel reads 4 B and writes 24 B per pixel; the deflection moves what tools/shear_bench.py counts for two inverse
transforms with the plain f32 store.  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from shear_bench import COL_CAP, HBM_BYTES_PER_S, LDS_POINTS, passes  # noqa: E402


def deflection_bytes(n):
    """Two inverses: filter + column passes (spectrum -> complex), then c2r row passes ending in the f32 map."""
    H, even = n // 2 + 1, n % 2 == 0
    row_c = 16 * (n * (n // 2) if even else (n + 1) // 2 * n)
    col_c = 16 * n * H
    mr, mc = passes(n // 2 if even else n, LDS_POINTS), passes(n, COL_CAP)
    one = (2 * col_c + 2 * col_c * (mc - 1)) + (col_c + 2 * row_c * (mr - 1) + 4 * n * n)
    return 2 * one


def timed(s, call, reps):
    for _ in range(3):
        call()
    s.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    s.synchronize()
    return (time.perf_counter() - t0) / reps


def report(nbytes, dt):
    floor = nbytes / HBM_BYTES_PER_S
    return {"ms_per_run": round(dt * 1e3, 3), "bytes": nbytes, "GB_per_s": round(nbytes / dt / 1e9, 1),
            "floor_ms": round(floor * 1e3, 3), "fraction_of_floor": round(floor / dt, 3),
            "times_the_floor": round(dt / floor, 2)}


def main(sizes=(4096, 16384), reps=20, angle=10.0):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            d = s.to_device(rng.standard_normal((n, n)).astype(np.float32))
            outs = [s.malloc(4 * n * n) for _ in range(slicer_amd.FD_COUNT)]
            try:
                with slicer_amd.Shear(s, n, angle) as sh:
                    sh.run(d)
                    t_alpha = timed(s, sh.deflection, reps)
                    phi = sh.device_map(slicer_amd.SHEAR_PHI)
                    spacing = np.deg2rad(angle) / n
                    t_fd = timed(s, lambda: slicer_amd.fd_run(s, phi, n, spacing, outs), reps)
            finally:
                s.free(d)
                for p in outs:
                    s.free(p)
            print(json.dumps({"npix": n, "slicer_shear_deflection": report(deflection_bytes(n), t_alpha),
                              "slicer_fd_derivatives": report(28 * n * n, t_fd)}), flush=True)


if __name__ == "__main__":
    main()
