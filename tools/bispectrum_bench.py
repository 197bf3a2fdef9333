"""Times slicer_bispectrum_run (forward r2c transform + B band inverses + the triple-product contraction) on a white-noise
map: 3 warm-up runs, then 20 timed runs.  The three parts are timed apart through slicer_profile_* (HIP events around
each); the wall time of a run is taken over a stream synchronisation.  The contraction is reported against its two
floors: the byte floor (the B f64 maps read once, B 8 npix^2 bytes at the HBM peak) and the arithmetic floor
(2 n_triples npix^2 f64 operations at the vector f64 peak).  One JSON line per case."""
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
F64_FLOPS = 78.6e12                            # MI355X peak vector f64 rate, public figure (computed floor, not measured)


def case(s, n, B, kind, reps=20, angle=10.0):
    rng = np.random.default_rng(n + B)
    d = s.to_device(rng.standard_normal((n, n)).astype(np.float32))
    edges = np.concatenate([[0.0], np.geomspace(1.0, 0.75 * n, B)])  # B bins; the first holds only m2 = 0, so it is empty
    try:
        t0 = time.perf_counter()
        with slicer_amd.Bispectrum(s, n, angle, edges=edges, triples=kind) as b:
            s.synchronize()
            create = time.perf_counter() - t0
            for _ in range(3):
                b.run(d)
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                b.run(d)
            s.synchronize()
            wall = (time.perf_counter() - t0) / reps
            s.profile_enable(True)
            s.profile_reset()
            for _ in range(reps):
                b.run(d)
            s.synchronize()
            prof = s.profile_get()
            s.profile_enable(False)
            T = b.triples.shape[0]
    finally:
        s.free(d)
    ms = {k: prof[k][1] / reps for k in ("bispectrum_fft", "bispectrum_band", "bispectrum", "bispectrum_finish")}
    byte_floor = B * 8 * n * n / HBM_BYTES_PER_S * 1e3
    flop_floor = 2.0 * T * n * n / F64_FLOPS * 1e3
    return {"npix": n, "bins": B, "triples": T, "kind": kind, "create_ms": round(create * 1e3, 3),
            "ms_per_run": round(wall * 1e3, 3), "forward_ms": round(ms["bispectrum_fft"], 3),
            "band_inverses_ms": round(ms["bispectrum_band"], 3), "contraction_ms": round(ms["bispectrum"], 3),
            "finish_ms": round(ms["bispectrum_finish"], 3), "contraction_byte_floor_ms": round(byte_floor, 4),
            "contraction_flop_floor_ms": round(flop_floor, 4),
            "contraction_fraction_of_floor": round(max(byte_floor, flop_floor) / ms["bispectrum"], 4)}


def main():
    with slicer_amd.Slicer(0) as s:
        for n, B, kind in ((1024, 8, "all"), (4096, 8, "all"), (4096, 32, "equilateral"), (4096, 32, "all")):
            print(json.dumps(case(s, n, B, kind)), flush=True)


if __name__ == "__main__":
    main()
