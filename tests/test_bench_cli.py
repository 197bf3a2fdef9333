"""bench.py's command line on one GPU: the JSON contract, and the one-run rehearsal of BOTH multi-rank layouts
 with a one-rank process group (SLICER_BENCH_FORCE_DIST=1: the same code path as N > 1 -- RCCL
communicator, StepGather, reduce_planes with the sync-free reduce meta -- on a single device)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


PLAIN = ["--side", "128", "--npix", "1024", "--files", "2", "--snapshots", "2", "--steps", "4", "--warmup", "1"]
# the roofline, the single-stream run and the reduce layouts are measured under --full only
SMALL = PLAIN + ["--full", "--cpu-baseline", "off", "--parity", "off", "--e2e", "off", "--profile-steps", "1"]


def test_one_gpu_line_has_the_contract_fields():
    d = _bench(SMALL)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["value"] > 0 and d["config"]["reduce_layout"] is None
    assert set(d["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    # one snapshot in flight by default; with --streams 2 the same steps on one stream are reported next to `value`
    assert d["config"]["streams"] == 1 and d["single_stream"] is None
    two = _bench(SMALL + ["--streams", "2"])
    assert two["config"]["streams"] == 2 and two["single_stream"]["value"] > 0 and two["value"] > 0


def test_one_run_times_the_step_layout_and_the_per_plane_reduce_layout():
    d = _bench(SMALL + ["--shard", "steps", "--reduce-layout", "on"], env={"SLICER_BENCH_FORCE_DIST": "1",
                                                                             "MASTER_PORT": "29533"})
    assert d["config"]["shard"] == "steps" and d["value"] > 0
    rl = d["config"]["reduce_layout"]
    assert d["config"]["collective"] is None and "no data-path collective" in d["config"]["maps"]
    for algo in ("rooted", "p2p", "steps_gather"):
        assert "error" not in rl[algo], rl[algo]
        assert rl[algo]["value"] > 0 and rl[algo]["ms_per_step"] > 0
        # one rank: both layouts deposit the same particles, so the rates must be of the same order (the reduce of a
        # one-rank group moves nothing); a sum that stalled the pipeline would show here
        # (this tiny job is 0.2 ms per step: the fixed costs of a collective round show; the headline job: 1.9 vs 2.0 ms)
        assert rl[algo]["value"] > 0.2 * d["value"], (rl[algo], d["value"])


@pytest.mark.parametrize("layout,port", [(["--shard", "files"], "29535"), (["--shard", "steps", "--gather", "on"], "29536")],
                         ids=["files", "gather"])
def test_no_overlap_layouts_run_under_torchs_default_stream(layout, port):
    """--no-overlap keeps ONE handle, set to torch's current stream -- the default stream, pointer 0, which leaves the
    handle on its own blocking stream (Slicer.set_stream).  reduce_planes accepts that pairing, since HIP orders a
    blocking stream with the legacy default stream (parallel.works_with_stream), and StepGather's sends read the maps
    behind plane_finalize for the same reason.  Before, `--shard files --no-overlap` ended in reduce_planes' "does not
    work on torch's current stream"."""
    d = _bench(SMALL + layout + ["--no-overlap"], env={"SLICER_BENCH_FORCE_DIST": "1", "MASTER_PORT": port})
    assert d["value"] > 0 and d["config"]["shard"] == layout[1]


def test_a_stuck_secondary_layout_cannot_take_the_main_number_down():
    """N > 1 runs time the reduce layouts after the main number; those collectives meet real multi-GPU hardware for the
    first time in the scaling run.  A watchdog prints the line with whatever finished and leaves if they do not finish in
    time -- here the time allowed is zero."""
    d = _bench(SMALL + ["--shard", "steps", "--reduce-layout", "on", "--secondary-timeout", "0.001"],
               env={"SLICER_BENCH_FORCE_DIST": "1", "MASTER_PORT": "29534"})
    assert d["value"] > 0 and d["config"]["shard"] == "steps"
    assert "cut off" in d["config"]["reduce_layout"]["error"]


def test_plain_line_times_the_steps_alone_and_dumps_the_last_step(tmp_path):
    d = _bench(PLAIN + ["--steps", "3", "--dump-outputs", str(tmp_path)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "f32"
    for k in ("roofline", "kernels", "parity", "e2e", "cpu_baseline", "single_stream"):
        assert d[k] is None, k
    maps, counts, sums = (np.load(tmp_path / f"{n}.npy") for n in ("maps", "counts", "map_sums"))
    assert maps.dtype == np.float32 and maps.shape == (4, 1024, 1024)
    assert counts.dtype == np.float64 and counts.shape == (4, 6) and counts[:, 1].sum() > 0
    assert np.allclose(sums, maps.sum(axis=(1, 2), dtype=np.float64), rtol=1e-12)
    # the map holds the mass of the step's deposits, less what TSC spreads past the edge from the one-pixel margin
    mass = counts[:, 1] * 0.0123
    assert np.all(sums <= mass * (1 + 1e-5)) and np.all(sums >= 0.98 * mass)


def test_dumped_outputs_repeat_with_the_same_arguments(tmp_path):
    """4096^2 maps are too large to dump whole: a fixed sample of pixels, the same in both runs."""
    args = ["--side", "128", "--npix", "4096", "--files", "2", "--snapshots", "2", "--steps", "2", "--warmup", "1"]
    for run in ("a", "b"):
        _bench(args + ["--dump-outputs", str(tmp_path / run)])
    a, b = ({n: np.load(tmp_path / r / f"{n}.npy") for n in ("counts", "map_sums", "maps_sample", "maps_sample_index")}
            for r in ("a", "b"))
    assert not (tmp_path / "a" / "maps.npy").exists()
    assert a["maps_sample"].dtype == np.float32 and a["maps_sample"].shape == (4, 1 << 21)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["maps_sample_index"], b["maps_sample_index"])
    # f32 atomics add in whatever order the hardware serves them: the last bits may differ, nothing more
    assert np.allclose(a["maps_sample"], b["maps_sample"], rtol=1e-5, atol=1e-9)
    assert np.allclose(a["map_sums"], b["map_sums"], rtol=1e-6)
