"""Times slicer_moments_run at 4096^2 and 16384^2, with levels = 0 and with the full pyramid, about every level's own
mean and about given centres: 3 warm-up runs, then 20 timed runs, wall time over a stream synchronisation.  Prints the
bytes each moves and the ratio to the HBM byte floor (computed at 6.3 TB/s, not measured): level 0 is read twice with
its own mean (the sum pass, then the moment pass) and once with a given centre; every further level is written once and
read once, 4 B a pixel.  The project's goal is 3x the floor.  One JSON line per size."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402


def moments_bytes(n, levels, own_mean):
    return 4 * ((2 if own_mean else 1) * n * n + sum(2 * (n >> l) ** 2 for l in range(1, levels + 1)))


def main(sizes=(4096, 16384), reps=20):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            d = s.to_device(rng.standard_normal((n, n)).astype(np.float32))
            out = {"npix": n}
            try:
                for levels in (0, int(np.log2(n))):
                    with slicer_amd.Moments(s, n, levels) as m:
                        for own in (True, False):
                            centres = None if own else np.zeros(levels + 1)
                            dt = timed(s, lambda: m.run(d, centres), reps)
                            out[f"levels_{levels}_{'own_mean' if own else 'given_centres'}"] = report(
                                moments_bytes(n, levels, own), dt)
            finally:
                s.free(d)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
