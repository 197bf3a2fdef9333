"""Times slicer_starlet_run and slicer_l1norm_run at 4096^2 on a white-noise map: 3 warm-up runs, then 20 timed runs,
wall time over a stream synchronisation, and the kernels apart from the per-kernel profile (HIP events) of the same 20
runs.  Each is set against its byte floor at 6.3 TB/s (computed, not measured):
  * a starlet level reads c_j once and writes w_{j+1} and c_{j+1}: 4 + 4 + 8 = 16 B a pixel for level 0 (f32 in),
    8 + 4 + 8 = 20 for a middle level, 8 + 4 + 4 = 16 for the last one (the coarse map instead of c_J); a transform of one
    level alone moves 4 + 4 + 4 = 12.  The profile has one name for each of the three (starlet_first, starlet_level,
    starlet_last), so handles of J = 2 ... 9 scales give every level on its own: level J - 1 as the last one, and
    level J - 2 as a middle one from the difference of starlet_level between J and J - 1;
  * the l1norm reads the map once: 4 B a pixel, at 64 bins (and at 1024, where the lanes of a wave take 32 turns).
For comparison, N12's row and column kernels on the same map (gauss, R = 16: 24 B a pixel) from the same profile.
The figures are reported, not gated.  One JSON line per case."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import HBM_BYTES_PER_S, timed  # noqa: E402


def profiled(s, call, reps):
    """({name: ms per run}, wall ms per run) of `call`."""
    dt = timed(s, call, reps)
    s.profile_reset()
    s.profile_enable(True)
    for _ in range(reps):
        call()
    s.synchronize()
    prof = s.profile_get()
    s.profile_enable(False)
    return {k: v[1] / reps for k, v in prof.items()}, dt * 1e3


def against(ms, bytes_per_pixel, n):
    floor = bytes_per_pixel * n * n / HBM_BYTES_PER_S * 1e3
    return {"ms": round(ms, 4), "floor_ms": round(floor, 4), "share_of_floor": round(floor / ms, 3)}


def main(n=4096, scales=8, reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((n, n), np.float32))
        try:
            level_sum = {}
            for J in range(2, scales + 2):
                with slicer_amd.Starlet(s, n, J) as st:
                    ms, wall = profiled(s, lambda: st.run(d), reps)
                    assert all(np.isfinite(st.read(j)).all() for j in (0, J))
                level_sum[J] = ms.get("starlet_level", 0.0)
                out = {"npix": n, "scales": J, "ms_per_run": round(wall, 4),
                       "level_0_first": against(ms["starlet_first"], 16, n),
                       f"level_{J - 1}_last": against(ms["starlet_last"], 16, n)}
                if J >= 3:
                    out[f"level_{J - 2}_middle"] = against(level_sum[J] - level_sum[J - 1], 20, n)
                if J == scales:
                    out["transform"] = against(wall, 16 + 20 * (J - 2) + 16, n)
                print(json.dumps(out), flush=True)
            for bins in (64, 1024):
                with slicer_amd.L1Norm(s, n, slicer_amd.peaks_edges(-4.0, 4.0, bins)) as l1:
                    ms, wall = profiled(s, lambda: l1.run(d), reps)
                    assert l1.read()["counts"].sum() > 0.99 * n * n
                print(json.dumps({"npix": n, "bins": bins, "ms_per_run": round(wall, 4), "l1norm": against(ms["l1norm"], 4, n),
                                  "l1norm_finish_ms": round(ms["l1norm_finish"], 4)}), flush=True)
            with slicer_amd.Smooth(s, n, "gauss", 4.0) as sm:
                ms, wall = profiled(s, lambda: sm.run(d), reps)
                print(json.dumps({"npix": n, "smooth": "gauss", "radius": sm.radius, "ms_per_run": round(wall, 4),
                                  "smooth_rows": against(ms["smooth_rows"], 12, n),
                                  "smooth_cols": against(ms["smooth_cols"], 12, n)}), flush=True)
        finally:
            s.free(d)


if __name__ == "__main__":
    main()
