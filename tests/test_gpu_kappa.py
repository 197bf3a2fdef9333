"""Device kappa accumulator (slicer_kappa_*, slicer_amd.Kappa) against numpy in f64."""
import numpy as np
import pytest

import kappa_np
import slicer_amd
from slicer_amd import synth


def check(got, ref):
    bound = 2.0 ** -23 * np.abs(ref) + 1e-6 * np.abs(ref).max()
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound), float(np.max(np.abs(got - ref) - bound))


def run_batches(s, npix, maps, coeff, batches):
    """maps [P, npix, npix] uploaded, added in `batches` (sizes), -> (kappa maps, plane means)."""
    S = coeff.shape[0]
    ptrs = [s.to_device(m) for m in maps]
    try:
        with slicer_amd.Kappa(s, npix, S) as k:
            p0 = 0
            for b in batches:
                k.add_device(ptrs[p0:p0 + b], coeff[:, p0:p0 + b].T)
                p0 += b
            assert p0 == len(maps)
            return np.stack([k.read(j) for j in range(S)]), k.plane_means()
    finally:
        for p in ptrs:
            s.free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("npix,n_src", [(100, 1), (100, 8), (100, 11), (37, 1), (37, 11), (4096, 11)])
def test_kappa_matches_numpy(npix, n_src):
    """Batches of 1, 4 and 8 maps; 11 sources take two launches per batch; 37^2 pixels leave a partial vector."""
    rng = np.random.default_rng(npix * 100 + n_src)
    batches = [1, 4, 8] if npix != 4096 else [4]
    P = sum(batches)
    maps = (rng.gamma(0.5, 2.0, (P, npix, npix)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-5, 1e-3, (n_src, P))
    coeff[:, rng.random(P) < 0.25] = 0.0          # planes behind some sources
    if n_src > 1:
        coeff[1] = 0.0                            # a source with no plane at all
    with slicer_amd.Slicer(0) as s:
        kap, means = run_batches(s, npix, maps, coeff, batches)
        ref = kappa_np.kappa(maps, coeff)
        for j in range(n_src):
            check(kap[j], ref[j])
        if n_src > 1:
            assert np.all(kap[1] == 0)
        mu = maps.astype(np.float64).reshape(P, -1).mean(axis=1)
        assert np.all(np.abs(means - mu) <= 1e-12 * np.abs(mu))
        # the same sequence again: bitwise the same maps
        kap2, means2 = run_batches(s, npix, maps, coeff, batches)
        assert np.array_equal(kap.view(np.uint32), kap2.view(np.uint32))
        assert np.array_equal(means.view(np.uint64), means2.view(np.uint64))


@pytest.mark.gpu
def test_kappa_state_and_argument_errors():
    with slicer_amd.Slicer(0) as s:
        k = slicer_amd.Kappa(s, 16, 2)
        d = s.to_device(np.ones((16, 16), np.float32))
        with pytest.raises(slicer_amd.SlicerError) as e:
            k.add_device([d] * 9, np.zeros((9, 2)))
        assert e.value.code == 2
        k.add_device([d], [[1.0, 0.0]])
        assert np.all(k.read(0) == 0) and np.all(k.read(1) == 0)   # a constant map has no fluctuation
        assert k.plane_means().tolist() == [1.0]
        # maps added after a finalize: kappa is refused until the next one
        k.add_device([d], [[1.0, 1.0]])
        p = slicer_amd.lensing.C.c_void_p()
        assert slicer_amd.lensing._L.slicer_kappa_device_map(k._kh, 0, slicer_amd.lensing.C.byref(p)) == 3
        k.finalize()
        assert k.device_map(1)
        k.close()
        s.free(d)


@pytest.mark.gpu
def test_kappa_of_a_real_deposit_pass():
    """Four TSC planes of one pass, read where slicer_plane_finalize left them, against kappa of the D2H copies."""
    box, npix, fov = 1000.0, 256, 0.25
    n = 1 << 18
    raw = synth.positions(0, n, box)
    ld = [3.0, 3.25, 3.5, 3.75]
    ld2 = [x + 0.25 for x in ld]
    w = slicer_amd.plane_weights(0.3, 0.7, -1.0, np.degrees(fov), npix, ld, ld2, [0.0] * 4, sources=[0.0012, 0.01])
    with slicer_amd.Slicer(0, max_chunk=1 << 20) as s:
        s.plane_begin(npix, fov, ld, ld2, mas=slicer_amd.MAS_TSC)
        s.file_begin([0, n, 0, 0, 0, 0], [0, 0.0123, 0, 0, 0, 0], box, (-1, 1, -1), 3, (0.3, 0.6, 0.1), 3.0)
        s.deposit_host(1, raw)
        s.file_end()
        s.plane_finalize()
        with slicer_amd.Kappa(s, npix, 2) as k:
            k.add(range(4), w["c"].T)
            kap = [k.read(0), k.read(1)]
            means = k.plane_means()
        maps = np.stack([s.plane_read(p, want_types=False)[0] for p in range(4)])
    assert maps.reshape(4, -1).max(axis=1).min() > 0
    ref = kappa_np.kappa(maps, w["c"])
    assert np.abs(ref[1]).max() > 0
    for j in range(2):
        check(kap[j], ref[j])
    mu = maps.astype(np.float64).reshape(4, -1).mean(axis=1)
    assert np.all(np.abs(means - mu) <= 1e-12 * mu)
