"""Times slicer_noise_run at 4096^2, with a map x and without (pure noise): 3 warm-up runs, then 20 timed runs, wall time
over a stream synchronisation, and the kernel alone from the per-kernel profile (HIP events) of the same 20 runs.  The
kernel is set against its floor (computed, not measured), the larger of
  * its bytes at 6.3 TB/s: 8 B a pixel (4 read, 4 written), 4 without x;
  * its f64 operations at 39.3e12 a second: half the 157.3 TFLOPS of the f32 vector units, which count a fused
    multiply-add as two.  They are counted from the generated gfx950 code of k_noise_add (the straight-line body of one
    block of four pixels; the library's log and sincospi bring their own fused multiply-adds): with x 134 additions and
    multiplications, 70 fused multiply-adds counted twice, 58 others (ldexp, conversions, comparisons, rcp, rsq, ...)
    = 332 a block, 83 a pixel; without x 130 + 2 * 70 + 54 = 324 a block, 81 a pixel.  The 19 integer multiplies of
    Philox's ten rounds (v_mul_hi_u32 / v_mul_lo_u32 / v_mad_u64_u32) are not in the count.
Reported, not gated.  One JSON line per case."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import HBM_BYTES_PER_S, timed  # noqa: E402

F64_OPS_PER_S = 39.3e12
BYTES_PER_PIXEL = {True: 8, False: 4}
F64_OPS_PER_BLOCK = {True: 332, False: 324}


def main(n=4096, reps=20, sigma=0.3):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((n, n), np.float32))
        try:
            with slicer_amd.Noise(s, n, 2024) as nz:
                for with_x in (True, False):
                    x = d if with_x else None
                    dt = timed(s, lambda: nz.run(x, sigma), reps)
                    s.profile_reset()
                    s.profile_enable(True)
                    for r in range(reps):
                        nz.run(x, sigma, 0, r)
                    s.synchronize()
                    launches, total_ms = s.profile_get()["noise_add"]
                    s.profile_enable(False)
                    assert launches == reps and np.isfinite(nz.read()).all()
                    ms = total_ms / launches
                    by_bytes = BYTES_PER_PIXEL[with_x] * n * n / HBM_BYTES_PER_S * 1e3
                    by_ops = F64_OPS_PER_BLOCK[with_x] * (n * n / 4) / F64_OPS_PER_S * 1e3
                    floor = max(by_bytes, by_ops)
                    print(json.dumps({"npix": n, "with_x": with_x, "ms_per_run": round(dt * 1e3, 4), "kernel_ms": round(ms, 4),
                                      "floor_bytes_ms": round(by_bytes, 4), "floor_f64_ms": round(by_ops, 4),
                                      "times_the_floor": round(ms / floor, 2),
                                      "Gpixel_per_s": round(n * n / (ms * 1e-3) / 1e9, 1)}), flush=True)
        finally:
            s.free(d)


if __name__ == "__main__":
    main()
