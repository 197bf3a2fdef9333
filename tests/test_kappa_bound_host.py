"""The derived bound of the device kappa maps (tests/kappa_np.py: kappa_bound) kept honest without
a GPU: a numpy emulation of the kernels' order of operations stays inside it with f64 accumulators and leaves it with
f32 accumulators, on the inputs of tests/test_gpu_kappa.py::test_kappa_matches_numpy."""
import numpy as np
import pytest

import kappa_np


@pytest.mark.parametrize("npix,n_src", [(100, 1), (100, 8), (100, 11), (37, 1), (37, 11)])
def test_bound_admits_f64_and_refuses_f32_accumulators(npix, n_src):
    maps, coeff, batches = kappa_np.planes_and_weights(npix, n_src)
    good = kappa_np.worst_ratio(kappa_np.emulate(maps, coeff, batches, np.float64), maps, coeff, len(batches))
    bad = kappa_np.worst_ratio(kappa_np.emulate(maps, coeff, batches, np.float32), maps, coeff, len(batches))
    print(f"npix {npix}, {n_src} sources: f64 accumulators {good:.4g}, f32 accumulators {bad:.4g} of the bound")
    assert good <= 1.0, good
    assert bad > 1.0, bad


def test_bound_is_dominated_by_the_f32_rounding():
    """The f64 terms are a small fraction of the f32 half-ulp wherever kappa is not a cancellation: the bound cannot
    hide an error of a few f32 ulps."""
    maps, coeff, batches = kappa_np.planes_and_weights(100, 11)
    centred, mu = kappa_np.centred_longdouble(maps)
    ref = kappa_np.kappa_longdouble(centred, coeff[0])
    bound = kappa_np.kappa_bound(ref, maps, mu, coeff[0], len(batches))
    typical = np.abs(ref) > 0.1 * np.abs(ref).max()
    assert float((bound[typical] / np.abs(ref[typical])).max()) < 2.0 ** -24 * 1.001


def test_mean_depth():
    assert kappa_np.mean_depth(16) == 19 and kappa_np.mean_depth(512) == 19
    assert kappa_np.mean_depth(513) == 20 and kappa_np.mean_depth(4096) == 18 + 64
