"""Device binned power spectra (slicer_power_*, slicer_amd.Power) against the f64 numpy
restatement in tests/power_np.py and against the shear handle's spectra."""
import numpy as np
import pytest

import power_np
import shear_np
import slicer_amd
from test_power_host import brute_force_cross


def log_edges(n):
    return np.concatenate([[0.0], np.geomspace(1.0, n * 0.75, 20)])


def maps_for(n, S):
    rng = np.random.default_rng(1000 + n)
    out = []
    for s in range(S):
        out.append(rng.standard_normal((n, n)).astype(np.float32) if s % 2 == 0 else shear_np.clustered(n, n + s))
    return out


def scaled_maps(n, S):
    """maps_for with every map times its own factor: no two pairs have the same spectrum, so a pair written to or read
    from another pair's place cannot agree by accident."""
    return [m * np.float32(0.5 + 0.173 * k) for k, m in enumerate(maps_for(n, S))]


def run_power(s, maps, angle, cross, edges=None, split=False, twice=False):
    n = maps[0].shape[0]
    s.set_option("shear_split", int(split))
    ptrs = [s.to_device(m) for m in maps]
    try:
        with slicer_amd.Power(s, n, angle, len(maps), cross=cross, edges=edges) as p:
            p.run(ptrs)
            got = p.read()
            idx = range(len(maps)) if cross else [len(maps) - 1]
            got["spectra"] = {k: p.spectrum(k) for k in idx}
            if twice:
                p.run(ptrs)
                got["again"] = p.read()["cl"]
            return got
    finally:
        for d in ptrs:
            s.free(d)
        s.set_option("shear_split", 0)


def shear_spectrum(s, kappa, angle, split):
    s.set_option("shear_split", int(split))
    d = s.to_device(kappa)
    try:
        with slicer_amd.Shear(s, kappa.shape[0], angle) as sh:
            sh.run(d)
            return sh.spectrum()
    finally:
        s.free(d)
        s.set_option("shear_split", 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check(s, maps, angle, edges, split):
    n, S = maps[0].shape[0], len(maps)
    ref_bins = slicer_amd.power_bins(n, edges)
    ell_f = slicer_amd.ell_fundamental(angle)
    auto = run_power(s, maps, angle, False, edges, split, twice=True)
    cross = run_power(s, maps, angle, True, edges, split, twice=True)
    for got in (auto, cross):
        assert np.array_equal(got["counts"], ref_bins["counts"])
        assert np.array_equal(bits(got["ell"]), bits(ref_bins["mean_radius"] * ell_f))
        assert np.array_equal(bits(got["again"]), bits(got["cl"]))  # bitwise repeatable
    for k in range(S):
        assert np.array_equal(bits(auto["cl"][k]), bits(cross["cl"][k, k])), k  # auto C_ss == cross C_ss
    # spectra: bitwise the shear handle's
    spectra = []
    for k in range(S):
        sp = shear_spectrum(s, maps[k], angle, split)
        assert np.array_equal(bits(cross["spectra"][k]), bits(sp)), k
        spectra.append(sp)
    assert np.array_equal(bits(auto["spectra"][S - 1]), bits(spectra[-1]))
    # binning: against the restatement's binning of the same spectra
    ref = power_np.power_of_spectra(spectra, angle, edges, cross=True)
    nz = ref["counts"] > 0
    assert np.array_equal(np.isnan(cross["cl"]), np.broadcast_to(~nz, cross["cl"].shape))
    err = np.abs(cross["cl"][..., nz] - ref["cl"][..., nz])
    bound = 1e-13 * ref["scale"][..., nz]
    assert np.all(err <= bound), float((err / bound).max())
    # against the restatement of the maps: the spectrum bound of N6, eps_s = 1e-12 log2(n) ||kappa_s||_2, propagated
    exact = [np.fft.rfft2(m.astype(np.float64)) for m in maps]
    eps = [1e-12 * np.log2(n) * np.linalg.norm(m.astype(np.float64)) for m in maps]
    counts, mags = power_np.binned_sums(n, power_np.default_edges(n) if edges is None else edges,
                                        [np.abs(x) for x in exact])
    exact_cl = power_np.power_of_spectra(exact, angle, edges, cross=True)["cl"]
    theta = np.radians(angle)
    norm = theta * theta / float(n) ** 4
    for a in range(S):
        for b in range(a, S):
            ma, mb = mags[a][nz] / counts[nz], mags[b][nz] / counts[nz]
            bnd = norm * (eps[a] * mb + eps[b] * ma + eps[a] * eps[b]) + 1e-13 * np.abs(exact_cl[a, b][nz])
            d = np.abs(cross["cl"][a, b][nz] - exact_cl[a, b][nz])
            assert np.all(d <= bnd), (a, b, float((d / bnd).max()))
    return cross


# A bin is cut into slices of about kSliceModes = 8192 modes, whole rows |j0| = a, and a workgroup walks the rows of its
# slice in chunks of 128.  Up to n = 100 a bin is one slice of one chunk.  1000 and 4096 have, with the default unit bins,
# one slice of up to 501 and 2049 rows (4 and 17 chunks) and, with log_edges, up to 26 and 444 slices a bin; the unit
# bins of 8505 and 16384 below have up to 2 and 4 slices of many chunks each.  The cap of a bin's slices at its rows
# needs more than 8192 modes a row, n > 8192 with one bin over most of the plane: no test here reaches it.
CASES = [(n, False) for n in (16, 30, 45, 49, 100, 1000, 4096)] + [(30, True), (45, True), (1024, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_power_matches_restatement(n, split):
    angle = 5.0 if n < 1000 else 10.0
    with slicer_amd.Slicer(0) as s:
        for edges in (None, log_edges(n)):
            check(s, maps_for(n, 3), angle, edges, split)
            if n <= 100:
                check(s, maps_for(n, 1), angle, edges, split)


# S > 8: k_power_bin<8> works on pairs of blocks of 8 sources.  9 and 17 leave a last block of one source, 24 gives
# three full blocks (block rows 1 and 2 of the triangle), 128 is the most the ABI takes (136 block pairs, 8256 pairs).
BLOCK_CASES = [(n, S) for n in (45, 100) for S in (8, 9, 16, 17, 24)] + [(16, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,S", BLOCK_CASES)
def test_cross_power_over_block_pairs(n, S):
    angle = 5.0
    maps = scaled_maps(n, S)
    with slicer_amd.Slicer(0) as s:
        for edges in (None, log_edges(n)):
            cross = check(s, maps, angle, edges, False)
            if n == 45:  # every pair against the plain double loop over the half plane, on the device's spectra
                cnt, cl, scale = brute_force_cross([cross["spectra"][k] for k in range(S)], angle,
                                                   power_np.default_edges(n) if edges is None else edges)
                assert np.array_equal(cross["counts"], cnt)
                nz = cnt > 0
                assert np.array_equal(np.isnan(cross["cl"]), np.isnan(cl))
                err = np.abs(cross["cl"] - cl)[..., nz]
                assert np.all(err <= 1e-13 * scale[..., nz]), float((err / (1e-13 * scale[..., nz])).max())


def one_large_map(n, seed):
    angle = 10.0
    kappa = shear_np.clustered(n, seed)
    with slicer_amd.Slicer(0) as s:
        got = run_power(s, [kappa], angle, False)
    assert np.array_equal(got["counts"], slicer_amd.power_bins(n)["counts"])
    exact = np.fft.rfft2(kappa.astype(np.float64))
    eps = 1e-12 * np.log2(n) * np.linalg.norm(kappa.astype(np.float64))
    assert float(np.abs(got["spectra"][0] - exact).max()) <= eps
    del got["spectra"]
    ref = power_np.power_of_spectra([exact], angle)
    edges = power_np.default_edges(n)
    counts, (mag,) = power_np.binned_sums(n, edges, [np.abs(exact)])
    del exact
    nz = counts > 0
    theta = np.radians(angle)
    bnd = theta ** 2 / float(n) ** 4 * (2 * eps * mag[nz] / counts[nz] + eps * eps) + 1e-13 * np.abs(ref["cl"][0][nz])
    d = np.abs(got["cl"][0][nz] - ref["cl"][0][nz])
    assert np.all(d <= bnd), float((d / bnd).max())


@pytest.mark.gpu
def test_power_16384_one_map():
    one_large_map(16384, 9)


@pytest.mark.gpu
def test_power_8505_one_map():
    """8505 = 3^5 5 7: the smallest size whose row transform takes two passes; slicer_power_create plans it itself."""
    one_large_map(8505, 11)


@pytest.mark.gpu
def test_run_kappa_equals_run_on_the_read_maps():
    n, angle = 64, 3.0
    rng = np.random.default_rng(5)
    planes = (rng.gamma(0.5, 2.0, (3, n, n)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-4, 1e-3, (2, 3))
    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(m) for m in planes]
        try:
            with slicer_amd.Kappa(s, n, 2) as k, slicer_amd.Power(s, n, angle, 2, cross=True) as p:
                k.add_device(ptrs, coeff.T)
                k.finalize()
                p.run_kappa(k)
                a = p.read()["cl"]
                read = [s.to_device(k.read(i)) for i in range(2)]
                try:
                    p.run(read)
                    assert np.array_equal(bits(a), bits(p.read()["cl"]))
                finally:
                    for d in read:
                        s.free(d)
                ref = power_np.power([k.read(0), k.read(1)], angle, cross=True)
                nz = ref["counts"] > 0
                np.testing.assert_allclose(a[..., nz], ref["cl"][..., nz], rtol=1e-9, atol=1e-12 * np.abs(a[..., nz]).max())
        finally:
            for d in ptrs:
                s.free(d)


@pytest.mark.gpu
def test_power_errors():
    with slicer_amd.Slicer(0) as s:
        def refused(code, *args, **kw):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Power(s, *args, **kw)
            assert e.value.code == code, (args, kw)
        for n in (37, 44, 0, 1, 16385):
            refused(6, n, 5.0, 1)  # SLICER_ERR_UNSUPPORTED
        for nm in (0, 129, -1):
            refused(6, 16, 5.0, nm)
        for edges in ([0.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("inf")], [0.0, float("nan")]):
            refused(2, 16, 5.0, 1, edges=edges)  # SLICER_ERR_ARG
        for angle in (0.0, -1.0, float("inf"), float("nan")):
            refused(2, 16, angle, 1)
        with slicer_amd.Power(s, 16, 5.0, 2) as p:
            for call in (p.read, lambda: p.spectrum(1)):
                with pytest.raises(slicer_amd.SlicerError) as e:
                    call()
                assert e.value.code == 3  # SLICER_ERR_STATE: nothing has run
            maps = [s.to_device(m) for m in maps_for(16, 2)]
            try:
                with pytest.raises(slicer_amd.SlicerError) as e:
                    p.run([maps[0], 0])
                assert e.value.code == 2
                p.run(maps)
                p.spectrum(1)
                with pytest.raises(slicer_amd.SlicerError) as e:
                    p.spectrum(0)  # auto mode keeps only the last map's spectrum
                assert e.value.code == 3
                with pytest.raises(slicer_amd.SlicerError) as e:
                    p.spectrum(2)
                assert e.value.code == 2
            finally:
                for d in maps:
                    s.free(d)
