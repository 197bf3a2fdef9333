"""Times slicer_scattering_run at J = 6, L = 4 on a 4096^2 white-noise map: 3 warm-up runs, then
10 timed runs, wall time over a stream synchronisation, and next to it the times of slicer_profile_* from a second set
of runs, per run and per profile name: scattering_first (khat and s0, then per (j1, l1) the filter, two inverses, the
sums and the forward transform of the modulus: 24 of those) and scattering_second (per (j1, l1) every (j2 > j1, l2):
the filter, two inverses and the sums, 240 of those in all).  A run makes J L (1 + (J - 1) L / 2) = 264 pairs of f64
inverses and 1 + (J - 1) L = 21 forward transforms (computed from J and L, like the numbers of the transforms above;
the times are measured).  Run by hand, never by a test.  One JSON line."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import timed  # noqa: E402

N, J, L, REPS = 4096, 6, 4, 10


def main(n=N, reps=REPS):
    rng = np.random.default_rng(0)
    pairs = J * L + L * L * J * (J - 1) // 2
    out = {"npix": n, "J": J, "L": L, "reps": reps, "inverse_pairs": pairs, "forwards": 1 + (J - 1) * L}
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(rng.standard_normal((n, n), np.float32))
        try:
            with slicer_amd.Scattering(s, n, J, L) as x:
                dt = timed(s, lambda: x.run(d), reps)
                r = x.read()
                s.profile_reset()
                s.profile_enable(True)
                for _ in range(reps):
                    x.run(d)
                s.synchronize()
                prof = s.profile_get()
                s.profile_enable(False)
        finally:
            s.free(d)
    out["ms_per_run"] = round(dt * 1e3, 2)
    out["ms_per_inverse_pair"] = round(dt * 1e3 / pairs, 3)
    for k in ("scattering_first", "scattering_second"):
        out[k] = {"scopes_per_run": prof[k][0] // reps, "ms_per_run": round(prof[k][1] / reps, 2)}
    out["s1_by_scale"] = [round(float(v), 5) for v in r["s1"].mean(axis=1)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
