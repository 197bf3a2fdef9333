"""Device kappa accumulator (slicer_kappa_*, slicer_amd.Kappa) against numpy in long double,
within the derived bound of tests/kappa_np.py."""
import numpy as np
import pytest

import kappa_np
import slicer_amd
from slicer_amd import synth


def check(got, maps, coeff, n_batches):
    """Every kappa map within the derived bound of kappa_np.kappa_bound (f64 accumulation, one f32 rounding) of the
    long-double reference."""
    worst = kappa_np.worst_ratio(got, maps, coeff, n_batches)
    print(f"kappa: worst |got - ref| / bound = {worst:.4g}")
    assert worst <= 1.0, worst


def check_means(means, maps):
    mu = kappa_np.centred_longdouble(maps)[1]
    err = np.abs(means.astype(np.longdouble) - mu).astype(np.float64)
    bound = kappa_np.mean_bound(maps)
    print(f"means: worst |got - ref| / bound = {float((err / bound).max()):.4g}")
    assert np.all(err <= bound), float((err / bound).max())


def upload(s, m, aligned=True):
    """-> (address to free, address of the map); not aligned: the map starts 4 bytes into its buffer."""
    if aligned:
        d = s.to_device(m)
        return d, d
    d = s.to_device(np.concatenate([np.zeros(1, np.float32), m.ravel()]))
    return d, d + 4


def run_batches(s, npix, maps, coeff, batches, unaligned=()):
    """maps [P, npix, npix] uploaded (those listed in `unaligned` off the 16-byte grid), added in `batches` (sizes),
    -> (kappa maps, plane means)."""
    S = coeff.shape[0]
    bufs = [upload(s, m, p not in unaligned) for p, m in enumerate(maps)]
    ptrs = [b[1] for b in bufs]
    assert all((p % 16 == 0) == (i not in unaligned) for i, p in enumerate(ptrs))
    try:
        with slicer_amd.Kappa(s, npix, S) as k:
            p0 = 0
            for b in batches:
                k.add_device(ptrs[p0:p0 + b], coeff[:, p0:p0 + b].T)
                p0 += b
            assert p0 == len(maps)
            return np.stack([k.read(j) for j in range(S)]), k.plane_means()
    finally:
        for b in bufs:
            s.free(b[0])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("npix,n_src", [(100, 1), (100, 8), (100, 11), (37, 1), (37, 11), (4096, 11)])
def test_kappa_matches_numpy(npix, n_src):
    """Batches of 1, 4 and 8 maps; 11 sources take two launches per batch; 37^2 pixels leave a partial vector."""
    maps, coeff, batches = kappa_np.planes_and_weights(npix, n_src)
    with slicer_amd.Slicer(0) as s:
        kap, means = run_batches(s, npix, maps, coeff, batches)
        check(kap, maps, coeff, len(batches))
        if n_src > 1:
            assert np.all(kap[1] == 0)
        check_means(means, maps)
        # the same sequence again: bitwise the same maps
        kap2, means2 = run_batches(s, npix, maps, coeff, batches)
        assert np.array_equal(bits(kap), bits(kap2))
        assert np.array_equal(bits(means), bits(means2))


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
    check(np.stack(kap), maps, w["c"], 1)
    check_means(means, maps)


@pytest.mark.gpu
@pytest.mark.parametrize("npix", [37, 100])
def test_kappa_of_unaligned_maps(npix):
    """A map pointer off the 16-byte grid (the ABI takes any const float *) sends its whole batch through the scalar
    loads of k_kappa_add<false>: bitwise the all-aligned run of the same data, and within the bound."""
    maps, coeff, batches = kappa_np.planes_and_weights(npix, 11)
    unaligned = {0, 2, 3, 7, 12}   # batch 1 of 1 all unaligned; batches of 4 and 8 mixed
    with slicer_amd.Slicer(0) as s:
        kap, means = run_batches(s, npix, maps, coeff, batches)
        kap_u, means_u = run_batches(s, npix, maps, coeff, batches, unaligned)
    assert np.array_equal(bits(kap), bits(kap_u))
    assert np.array_equal(bits(means), bits(means_u))
    check(kap_u, maps, coeff, len(batches))
    check_means(means_u, maps)


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [2, 9])
def test_kappa_of_more_than_1024_maps(n_src):
    """130 batches of 8 maps: the means array (1024 slots at first) grows in mid-sequence."""
    npix, n_up, n_batches = 16, 5, 130
    rng = np.random.default_rng(1040 + n_src)
    up = (rng.gamma(0.5, 2.0, (n_up, npix, npix)) * 3.0).astype(np.float32)
    P = 8 * n_batches
    which = np.arange(P) % n_up
    coeff = rng.uniform(1e-5, 1e-3, (n_src, P))
    coeff[:, rng.random(P) < 0.25] = 0.0

    def sequence(s, ptrs):
        with slicer_amd.Kappa(s, npix, n_src) as k:
            for b in range(n_batches):
                sl = slice(8 * b, 8 * b + 8)
                k.add_device([ptrs[i] for i in which[sl]], coeff[:, sl].T)
            return np.stack([k.read(j) for j in range(n_src)]), k.plane_means()

    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(m) for m in up]
        try:
            kap, means = sequence(s, ptrs)
            kap2, means2 = sequence(s, ptrs)
        finally:
            for p in ptrs:
                s.free(p)
    maps = up[which]
    assert means.shape == (1040,)
    check_means(means, maps)
    for i in range(n_up):      # the same map gives the same mean wherever it stands in the sequence
        assert np.unique(bits(means[which == i])).size == 1
    check(kap, maps, coeff, n_batches)
    assert np.array_equal(bits(kap), bits(kap2)) and np.array_equal(bits(means), bits(means2))


@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [8, 9, 16, 17])
def test_kappa_source_group_edges(n_src):
    """Sources go to the kernels in groups of 8: a full last group (8, 16), a group of one (9, 17); a batch whose
    coefficients of the second group are all zero (that launch is skipped) and one with no non-zero coefficient at all
    (only the partial sums and the means are written)."""
    npix, batches = 37, [3, 8, 4, 2]
    rng = np.random.default_rng(370 + n_src)
    P = sum(batches)
    maps = (rng.gamma(0.5, 2.0, (P, npix, npix)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-5, 1e-3, (n_src, P))
    coeff[8:16, 3:11] = 0.0    # batch 2: nothing for the second group
    coeff[:, 11:15] = 0.0      # batch 3: nothing for anybody
    with slicer_amd.Slicer(0) as s:
        kap, means = run_batches(s, npix, maps, coeff, batches)
        kap2, means2 = run_batches(s, npix, maps, coeff, batches)
    check(kap, maps, coeff, len(batches))
    check_means(means, maps)
    assert np.array_equal(bits(kap), bits(kap2)) and np.array_equal(bits(means), bits(means2))
