"""Times slicer_smooth_run at 4096^2 on a white-noise map, sigma = 4, 16 and 32 pixels at truncate 4 (R = 16, 64, 128),
both kinds: 3 warm-up runs, then 20 timed runs, wall time over a stream synchronisation, and the two kernels apart from
the per-kernel profile (HIP events) of the same 20 runs.  Each kernel is set against its floor (computed, not measured),
the larger of
  * its bytes at 6.3 TB/s: the row kernel reads 4 B a pixel and writes 8 (GAUSS: T) or 16 (MAP: D and G), the column
    kernel reads those and writes 4, so a run moves 24 or 40 B a pixel;
  * its f64 operations, counted from the code (an addition or a multiplication is one operation, nothing is fused), at
    39.3e12 a second: half the 157.3 TFLOPS of the f32 vector units, which count a fused multiply-add as two.  Per
    pixel the row kernel does 3 R + 1 (GAUSS) or 5 R + 3 (MAP: the pair sum is shared by the g and the h chain), the
    column kernel 3 R + 3 (GAUSS, the division counted as one) or 6 R + 4 (MAP: D and G are different lines).
The project's goal is 3x the floor; it is reported here, not gated.  One JSON line per case."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import HBM_BYTES_PER_S, timed  # noqa: E402

F64_OPS_PER_S = 39.3e12
BYTES = {"gauss": {"smooth_rows": 12, "smooth_cols": 12}, "map": {"smooth_rows": 20, "smooth_cols": 20}}


def ops(kind, R):
    if kind == "gauss":
        return {"smooth_rows": 3 * R + 1, "smooth_cols": 3 * R + 3}
    return {"smooth_rows": 5 * R + 3, "smooth_cols": 6 * R + 4}


def main(n=4096, sigmas=(4.0, 16.0, 32.0), reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((n, n), np.float32))
        try:
            for kind in ("gauss", "map"):
                for sigma in sigmas:
                    with slicer_amd.Smooth(s, n, kind, sigma) as sm:
                        R = sm.radius
                        dt = timed(s, lambda: sm.run(d), reps)
                        s.profile_reset()
                        s.profile_enable(True)
                        for _ in range(reps):
                            sm.run(d)
                        s.synchronize()
                        prof = s.profile_get()
                        s.profile_enable(False)
                        assert np.isfinite(sm.read()).all()
                    out = {"npix": n, "kind": kind, "sigma_pix": sigma, "radius": R, "ms_per_run": round(dt * 1e3, 3)}
                    floor_run = 0.0
                    for name in ("smooth_rows", "smooth_cols"):
                        launches, total_ms = prof[name]
                        assert launches == reps
                        ms = total_ms / launches
                        by_bytes = BYTES[kind][name] * n * n / HBM_BYTES_PER_S * 1e3
                        by_ops = ops(kind, R)[name] * n * n / F64_OPS_PER_S * 1e3
                        floor = max(by_bytes, by_ops)
                        floor_run += floor
                        out[name] = {"ms": round(ms, 3), "floor_bytes_ms": round(by_bytes, 3), "floor_f64_ms": round(by_ops, 3),
                                     "times_the_floor": round(ms / floor, 2)}
                    out["floor_ms"] = round(floor_run, 3)
                    out["times_the_floor"] = round(dt * 1e3 / floor_run, 2)
                    print(json.dumps(out), flush=True)
        finally:
            s.free(d)


if __name__ == "__main__":
    main()
