"""Times slicer_shear_run (forward r2c + phi, gamma1, gamma2 inverses, |gamma|) at 4096^2 and 16384^2: 3 warm-up runs,
then 20 timed runs, wall time over a stream synchronisation.  Prints the bytes the pass structure moves (every pass
reads and writes its whole array once), the fraction of the HBM byte floor, and the same
computation with scipy.fft in f64 on 16 workers for context.  One JSON line per size."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # MI355X peak HBM bandwidth (computed floor, not measured)
LDS_POINTS, COL_CAP = 8192, 1024  # slicer_fft.hip: kLdsPoints, kColCap


def passes(L, cap):
    m, rem = 0, L
    while True:
        R = max([d for d in range(2, min(rem, cap) + 1) if rem % d == 0] or [1])
        m, rem = m + 1, rem // R
        if rem <= 1:
            return m


def bytes_moved(n):
    H, even = n // 2 + 1, n % 2 == 0
    row_c = 16 * (n * (n // 2) if even else (n + 1) // 2 * n)  # complex f64 rows (n/2-point or paired n-point)
    col_c = 16 * n * H
    mr, mc = passes(n // 2 if even else n, LDS_POINTS), passes(n, COL_CAP)
    fwd = 4 * n * n + row_c + 2 * row_c * (mr - 1) + row_c + col_c + 2 * col_c * (mc - 1)
    inv_cols = 3 * (2 * col_c + 2 * col_c * (mc - 1))
    inv_rows = 3 * (col_c + 2 * row_c * (mr - 1)) + 4 * n * n + row_c + (row_c + 12 * n * n)
    return fwd + inv_cols + inv_rows, mr, mc


def scipy_ms(kappa, angle, reps=3):
    import scipy.fft as sf
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import shear_np
    n = kappa.shape[0]
    fphi, fg1, fg2 = shear_np.filters(n, angle)
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        k = sf.rfft2(kappa.astype(np.float64), workers=16)
        maps = [sf.irfft2(k * f, s=(n, n), workers=16) for f in (fphi, fg1, fg2)]
        np.sqrt(maps[1] ** 2 + maps[2] ** 2)
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main(sizes=(4096, 16384), reps=20, angle=10.0):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            kappa = rng.standard_normal((n, n)).astype(np.float32)
            d = s.to_device(kappa)
            with slicer_amd.Shear(s, n, angle) as sh:
                for _ in range(3):
                    sh.run(d)
                s.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    sh.run(d)
                s.synchronize()
                dt = (time.perf_counter() - t0) / reps
            s.free(d)
            nbytes, mr, mc = bytes_moved(n)
            print(json.dumps({"npix": n, "row_passes": mr, "col_passes": mc, "ms_per_run": round(dt * 1e3, 3),
                              "bytes": nbytes, "GB_per_s": round(nbytes / dt / 1e9, 1),
                              "floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 3),
                              "fraction_of_floor": round(nbytes / HBM_BYTES_PER_S / dt, 3),
                              "scipy_f64_16_workers_ms": round(scipy_ms(kappa, angle, 1 if n > 8192 else 3), 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
