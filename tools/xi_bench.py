"""Times the real-space two-point handle on 4096^2 white-noise maps with L = 1024 (P = 5120) and
32 log bins under a 70 % random 0/1 mask: slicer_xi_set_weights (it waits for the stream itself), a spin-0 auto run of
one field and a spin-2 run of one field; 2 warm-up runs, then 5 timed ones, wall time over a stream synchronisation.

Each time is set against a byte floor, the bytes the step must move if every array crossed HBM once per use, with
T = 8 P^2 (one f64 map, and to within a column one half-plane spectrum), W = 2 L + 1:
  pad to f64          4 n^2 + T            pad to f32         4 n^2 + T / 2
  forward of f32      T / 2 + 3 T          forward of a product  2 T + 3 T   (input, row output written and read, spectrum)
  spectrum            (inputs + 1) T       inverse            4 T            binning  8 W^2 per window read
  set_weights  4 n^2 (the check) + both pads + forward of f32 + spectrum of 1 + inverse + binning + the window copy 16 W^2
  spin-0 run   pad + forward of a product + spectrum of 1 + inverse + binning
  spin-2 run   2 (pad + forward of a product) + 3 (spectrum of 2 + inverse) + binning of 3 windows
and reported as the bandwidth the time implies for those bytes (the multi-pass transforms of P = 5120 move more than the
floor counts: longer lines take two passes).  One JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slicer_amd  # noqa: E402

N, L, BINS, WARM, REPS = 4096, 1024, 32, 2, 5


def timed(s, call, reps=REPS):
    for _ in range(WARM):
        call()
    s.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    s.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    edges = np.concatenate([[0.0], np.geomspace(1.0, float(L), BINS)])
    P = slicer_amd.xi_bins(N, edges)["padded"]
    T, n2, W2 = 8.0 * P * P, float(N) * N, float(2 * L + 1) ** 2
    pad, fwd_prod, inverse = 4 * n2 + T, 5 * T, 4 * T
    floors = {"set_weights": 4 * n2 + pad + (4 * n2 + T / 2) + 3.5 * T + 2 * T + inverse + 8 * W2 + 16 * W2,
              "spin0_run": pad + fwd_prod + 2 * T + inverse + 8 * W2,
              "spin2_run": 2 * (pad + fwd_prod) + 3 * (3 * T + inverse) + 24 * W2}
    rng = np.random.default_rng(N)
    out = {"npix": N, "max_lag": L, "padded": P, "bins": BINS}
    with slicer_amd.Slicer(0) as s:
        d = [s.to_device(rng.standard_normal((N, N)).astype(np.float32)) for _ in range(2)]
        w = s.to_device((rng.random((N, N)) < 0.7).astype(np.float32))
        try:
            with slicer_amd.Xi(s, N, 0, 1, edges) as x:
                ms = {"set_weights": timed(s, lambda: x.set_weights(w)), "spin0_run": timed(s, lambda: x.run(d[:1]))}
            with slicer_amd.Xi(s, N, 2, 1, edges) as x:
                x.set_weights(w)
                ms["spin2_run"] = timed(s, lambda: x.run(d))
        finally:
            for p in d + [w]:
                s.free(p)
    for k, t in ms.items():
        out[k + "_ms"] = round(t, 3)
        out[k + "_floor_gb"] = round(floors[k] / 1e9, 3)
        out[k + "_gb_per_s"] = round(floors[k] / 1e9 / (t / 1e3), 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
