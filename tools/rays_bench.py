"""Times slicer_rays_step (the first step, which builds the start state, and a later one) and slicer_rays_observe (all
six outputs) at 4096^2 and 16384^2 on white-noise maps whose deflections scatter the rays by about a pixel: 3 warm-up
runs, then 20 timed runs, wall time over a stream synchronisation.  Prints the ratio to the HBM byte floor (computed at
6.3 TB/s, not measured): a step reads and writes the twelve f64 state arrays and gathers five f32
maps, 96 + 96 + 20 = 212 B a ray; the first step reads no state, 116 B; observe reads the state arrays behind its
outputs, all twelve for all six, and writes 4 B an output, 96 + 24 = 120 B.  The project's goal is 3x the floor; it is
reported here, not gated.  One JSON line per size."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402
from deflection_bench import report, timed  # noqa: E402


def main(sizes=(4096, 16384), reps=20, spacing=1e-4):
    rng = np.random.default_rng(0)
    with slicer_amd.Slicer(0) as s:
        for n in sizes:
            scale = (spacing, spacing, 0.02, 0.02, 0.02)
            maps = [s.to_device(rng.standard_normal((n, n), np.float32) * np.float32(a)) for a in scale]
            outs = [s.malloc(4 * n * n) for _ in range(slicer_amd.RAYS_COUNT)]
            chi = [0.0]

            def first():
                rays.reset()
                rays.step(1.0, *maps)

            def later():  # (chi only has to grow; w tends to 0 and the rays stay where the first steps left them)
                chi[0] += 1.0
                rays.step(1.0 + chi[0], *maps)

            try:
                with slicer_amd.Rays(s, n, spacing) as rays:
                    t_first = timed(s, first, reps)
                    t_step = timed(s, later, reps)
                    t_obs = timed(s, lambda: rays.observe_device(1e3, outs), reps)
            finally:
                for p in maps + outs:
                    s.free(p)
            print(json.dumps({"npix": n, "first_step": report(116 * n * n, t_first), "step": report(212 * n * n, t_step),
                              "observe": report(120 * n * n, t_obs)}), flush=True)


if __name__ == "__main__":
    main()
