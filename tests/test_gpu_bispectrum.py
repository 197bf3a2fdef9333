"""Device binned bispectra (slicer_bispectrum_*, slicer_amd.Bispectrum) against the f64 numpy
restatement in tests/bispectrum_np.py, staged like the power spectra's pin: (a) the spectrum is bitwise the shear
handle's, (b) the band maps against irfft2 of the device's own spectrum, (c) the sums against math.fsum over the
device's own maps, (d) the triangle counts against the exact ones, (e) NaN exactly where there is no triangle, (f) end
to end against the restatement of the f32 map."""
import math

import numpy as np
import pytest

import bispectrum_np
import shear_np
import slicer_amd
from test_gpu_power import bits, shear_spectrum


def log_edges(n):
    return np.concatenate([[0.0], np.geomspace(1.0, n * 0.75, 8)])


def narrow_edges(n):
    """Six bins one unit wide from 2 (all at or below n / 3 from n = 24 on: no triangle closes modulo n only there)."""
    return 2.0 + np.arange(7.0)


def maps_for(n):
    """As test_gpu_power.maps_for: white noise, and a clustered (Gamma-distributed, so skewed: B != 0) field."""
    rng = np.random.default_rng(1000 + n)
    return [rng.standard_normal((n, n)).astype(np.float32), shear_np.clustered(n, n + 1)]


def triples_for(n, B):
    """All triples on the small maps; on the large ones a list that keeps the fsum of (c) short: equilateral, folded,
    squeezed and mixed ones over the whole range of bins."""
    if n <= 100:
        return bispectrum_np.all_triples(B)
    rows = [(1, 1, 1), (B - 1, B - 1, B - 1), (1, B - 1, B - 1), (1, 1, 2), (1, 2, 3), (2, 2, 4), (B - 3, B - 2, B - 1),
            (3, 3, 3), (1, B - 2, B - 1), (0, 1, 1)]
    return np.array(sorted(set(r for r in rows if 0 <= r[0] <= r[1] <= r[2] < B)), np.int32)


def exact_counts(n, edges, triples):
    """The exact T: by enumeration on the host where that is affordable, else the restatement's rounded (its own error
    obeys the bound of (d), which stays below 0.5 at every size here)."""
    if n <= 100:
        return slicer_amd.bispectrum_triangles(n, edges, triples)
    return np.rint(bispectrum_np.triangles(n, edges, triples)).astype(np.int64)


def run_bispectrum(s, d_map, n, angle, edges, triples, split=False, maps=False):
    s.set_option("shear_split", int(split))
    try:
        with slicer_amd.Bispectrum(s, n, angle, edges=edges, triples=triples) as b:
            early = b.triangles()
            b.run(d_map)
            got = b.read()
            assert np.array_equal(bits(early), bits(got["triangles"]))
            got["spectrum"] = b.spectrum()
            if maps:
                got["F"] = np.stack([b.read_map(k) for k in range(len(edges) - 1)])
            return got
    finally:
        s.set_option("shear_split", 0)


def check(s, kappa, angle, edges, split):
    n = kappa.shape[0]
    B = len(edges) - 1
    tr = triples_for(n, B)
    lg = np.log2(n)
    d = s.to_device(kappa)
    try:
        got = run_bispectrum(s, d, n, angle, edges, tr, split, maps=True)
    finally:
        s.free(d)
    assert np.array_equal(got["triples"], tr)
    # (a) the spectrum: bitwise the shear handle's
    assert np.array_equal(bits(got["spectrum"]), bits(shear_spectrum(s, kappa, angle, split)))
    # (b) the band maps: N6's forward bound carried through Parseval
    refF = bispectrum_np.band_maps(got["spectrum"], n, edges)
    for b in range(B):
        rms = np.sqrt(np.mean(refF[b] ** 2))
        err = np.abs(got["F"][b] - refF[b]).max()
        print(f"(b) n={n} bin={b} err={err:.3e} bound={1e-12 * lg * rms:.3e}")
        assert err <= 1e-12 * lg * rms, (b, err, rms)
    # (c) the sums: N7's bin-sum bound, against fsum over the products of the device's own maps
    for t, (i, j, k) in enumerate(tr):
        prod = ((got["F"][i] * got["F"][j]) * got["F"][k]).ravel()
        want, scale = math.fsum(prod), math.fsum(np.abs(prod))
        print(f"(c) n={n} triple={i},{j},{k} err={abs(got['sums'][t] - want):.3e} bound={1e-13 * scale:.3e}")
        assert abs(got["sums"][t] - want) <= 1e-13 * scale, (i, j, k)
    # (d) the triangle counts, (e) NaN exactly where there is none
    N = bispectrum_np.full_plane_counts(n, edges).astype(np.float64)
    exact = exact_counts(n, edges, tr)
    bound_t = 3e-12 * lg * np.sqrt(N[tr[:, 0]] * N[tr[:, 1]] * N[tr[:, 2]])
    assert bound_t.max() < 0.5
    err_t = np.abs(got["triangles"] - exact)
    print(f"(d) n={n} worst err/bound={np.max(err_t / np.maximum(bound_t, 1e-300)):.3e} bound max={bound_t.max():.3e}")
    assert np.all(err_t <= bound_t), float(np.max(err_t / np.maximum(bound_t, 1e-300)))
    assert np.array_equal(np.isnan(got["b"]), exact == 0)
    # (f) end to end against the restatement of the f32 map
    ref = bispectrum_np.bispectrum(kappa, angle, edges, tr)
    assert np.array_equal(np.isnan(ref["b"]), exact == 0)
    theta = np.radians(angle)
    eps = 1e-12 * lg * np.linalg.norm(kappa.astype(np.float64))
    r = np.sqrt(np.mean(ref["F"] ** 2, axis=(1, 2)))
    e = eps * N / float(n) ** 2 + 1e-12 * lg * r
    i, j, k = tr[:, 0], tr[:, 1], tr[:, 2]
    nz = exact > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        bound = theta ** 4 / float(n) ** 2 / ref["triangles"] * float(n) ** 2 * (e[i] * r[j] * r[k] + r[i] * e[j] * r[k] +
                                                                                  r[i] * r[j] * e[k]) + 1e-13 * np.abs(ref["b"])
    err = np.abs(got["b"] - ref["b"])
    print(f"(f) n={n} worst err/bound={np.max(err[nz] / bound[nz]):.3e}")
    assert np.all(err[nz] <= bound[nz]), float(np.max(err[nz] / bound[nz]))
    assert np.any(np.abs(got["b"][nz]) > 0)
    return got


CASES = [(n, False) for n in (16, 30, 45, 49, 100, 1000)] + [(30, True), (45, True), (1024, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_bispectrum_matches_restatement(n, split):
    angle = 5.0 if n < 1000 else 10.0
    with slicer_amd.Slicer(0) as s:
        white, clustered = maps_for(n)
        check(s, white, angle, log_edges(n), split)
        check(s, clustered, angle, narrow_edges(n), split)
        if n <= 100:  # (the large maps take each set once)
            check(s, white, angle, narrow_edges(n), split)
            check(s, clustered, angle, log_edges(n), split)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [30, 1024])
def test_split_and_unsplit_give_equal_bits(n):
    """b, triangles, sums and the band maps have the same bits under shear_split 0 and 1.  The reported spectrum is the
    exception the contract itself makes: under each setting it is bitwise the shear handle's (stage (a) of the cases
    above), and the shear handle's own spectra differ between the settings in the last bits (the split reorders the
    butterflies), so it can only be checked to be the shear handle's, here under both."""
    kappa = maps_for(n)[1]
    edges = log_edges(n)
    tr = triples_for(n, 8)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            a = run_bispectrum(s, d, n, 5.0, edges, tr, False, maps=n == 30)
            b = run_bispectrum(s, d, n, 5.0, edges, tr, True, maps=n == 30)
        finally:
            s.free(d)
        for got, split in ((a, False), (b, True)):
            assert np.array_equal(bits(got["spectrum"]), bits(shear_spectrum(s, kappa, 5.0, split))), split
    keys = ("b", "sums", "triangles") + (("F",) if n == 30 else ())
    for key in keys:
        x, y = np.nan_to_num(a[key]), np.nan_to_num(b[key])
        print(f"split n={n} {key}: differing values {int(np.sum(bits(a[key]) != bits(b[key])))} of {x.size}, "
              f"max |d| / max |x| = {float(np.abs(x - y).max() / np.abs(x).max()):.3e}")
    for key in keys:
        assert np.array_equal(bits(a[key]), bits(b[key])), key


@pytest.mark.gpu
def test_two_pass_column_chain():
    """n = 2048 is the smallest power of two whose column transform takes two passes without shear_split (at most 1024
    points a pass): the band load then feeds a pass that stores to an intermediate.  Two unit bins and their four
    triples; stages (a), (b) and (c) as above."""
    n, angle = 2048, 10.0
    edges = np.array([2.0, 3.0, 4.0])
    tr = bispectrum_np.all_triples(2)
    kappa = shear_np.clustered(n, 7)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            got = run_bispectrum(s, d, n, angle, edges, tr, maps=True)
        finally:
            s.free(d)
        assert np.array_equal(bits(got["spectrum"]), bits(shear_spectrum(s, kappa, angle, False)))
    refF = bispectrum_np.band_maps(got["spectrum"], n, edges)
    for b in range(2):
        rms = np.sqrt(np.mean(refF[b] ** 2))
        assert rms > 0 and np.abs(got["F"][b] - refF[b]).max() <= 1e-12 * np.log2(n) * rms, b
    for t, (i, j, k) in enumerate(tr):
        prod = ((got["F"][i] * got["F"][j]) * got["F"][k]).ravel()
        assert abs(got["sums"][t] - math.fsum(prod)) <= 1e-13 * math.fsum(np.abs(prod)), (i, j, k)
    exact = np.rint(bispectrum_np.triangles(n, edges, tr)).astype(np.int64)
    assert np.array_equal(np.rint(got["triangles"]).astype(np.int64), exact) and np.all(exact > 0)


def chunking(n):
    """(pixels of a chunk, chunks) of k_bispectrum as slicer_bispectrum_create of slicer_amd/csrc/slicer_bispectrum.hip
    sets them: at most kMaxChunks = 1024 chunks of at least kMinChunk = 4096 pixels, a multiple of 64."""
    npix2 = n * n
    want = min(1024, (npix2 + 4095) // 4096)
    chunk = ((npix2 + want - 1) // want + 63) // 64 * 64
    return chunk, (npix2 + chunk - 1) // chunk


# A lane sums its products in blocks of kInner = 64 wave-wide steps, and a chunk has chunk / 64 steps: up to n = 2048
# (1024 chunks of 4096) every chunk is one block, only past it a second one adds into the accumulators in LDS.  One chunk
# (n <= 64), fewer chunks than the 64 lanes of k_bispectrum_finish (100: 3), more (1000: 245, four a lane, the last two
# lanes idle) and a ragged last chunk (every size but the powers of two) are met by CASES.
assert all(chunking(n)[0] <= 64 * 64 for n in (16, 30, 45, 49, 100, 1000, 1024, 2048)) and chunking(2048) == (4096, 1024)
assert [chunking(n)[1] for n in (49, 100, 1000, 1024)] == [1, 3, 245, 256]
assert chunking(2058) == (4160, 1019) and 2058 * 2058 - 1018 * 4160 == 484  # 65 steps; the last chunk is ragged


@pytest.mark.gpu
def test_chunks_past_one_inner_block():
    """n = 2058 = 2 * 3 * 7^3 is the smallest size the transform takes past 2048: kMaxChunks caps the chunks at 1024, a
    chunk grows to 4160 pixels and its 65th step is a second inner block.  Two unit bins and their four triples; stage
    (c) as above, and the triangle counts, which the same contraction forms at create."""
    n, angle = 2058, 10.0
    edges = np.array([2.0, 3.0, 4.0])
    tr = bispectrum_np.all_triples(2)
    kappa = shear_np.clustered(n, 11)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            got = run_bispectrum(s, d, n, angle, edges, tr, maps=True)
        finally:
            s.free(d)
    for t, (i, j, k) in enumerate(tr):
        prod = ((got["F"][i] * got["F"][j]) * got["F"][k]).ravel()
        want, scale = math.fsum(prod), math.fsum(np.abs(prod))
        assert scale > 0 and abs(got["sums"][t] - want) <= 1e-13 * scale, (i, j, k)
    exact = np.rint(bispectrum_np.triangles(n, edges, tr)).astype(np.int64)
    assert np.array_equal(np.rint(got["triangles"]).astype(np.int64), exact) and np.all(exact > 0)


@pytest.mark.gpu
def test_runs_repeat_and_carry_nothing_over():
    n, angle = 45, 5.0
    edges = log_edges(n)
    first, second = maps_for(n)
    with slicer_amd.Slicer(0) as s:
        d1, d2 = s.to_device(first), s.to_device(second)
        try:
            with slicer_amd.Bispectrum(s, n, angle, edges=edges) as b:
                b.run(d1)
                a = b.read()
                b.run(d1)
                again = b.read()
                b.run(d2)
                other = b.read()
                other_map = b.read_map(3)
            with slicer_amd.Bispectrum(s, n, angle, edges=edges) as b:
                b.run(d2)
                fresh = b.read()
                fresh_map = b.read_map(3)
        finally:
            s.free(d1)
            s.free(d2)
    for key in ("b", "sums", "triangles"):
        assert np.array_equal(bits(a[key]), bits(again[key])), key
        assert np.array_equal(bits(other[key]), bits(fresh[key])), key
    assert np.array_equal(bits(other_map), bits(fresh_map))
    assert not np.array_equal(bits(a["sums"]), bits(other["sums"]))


@pytest.mark.gpu
def test_a_triple_alone_has_the_bits_it_has_in_the_full_list():
    n, angle = 45, 5.0
    edges = log_edges(n)
    kappa = maps_for(n)[1]
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            full = run_bispectrum(s, d, n, angle, edges, "all")
            for t, row in enumerate(full["triples"]):
                one = run_bispectrum(s, d, n, angle, edges, row[None, :])
                for key in ("b", "sums", "triangles"):
                    assert np.array_equal(bits(one[key]), bits(full[key][t:t + 1])), (row, key)
        finally:
            s.free(d)


@pytest.mark.gpu
def test_triple_list_shapes():
    n, angle = 16, 5.0
    kappa = maps_for(n)[1]
    edges = np.linspace(0.5, 11.5, 33)  # 32 bins
    every = bispectrum_np.all_triples(32)
    assert every.shape[0] == 5984
    ref = bispectrum_np.bispectrum(kappa, angle, edges, every)
    exact = slicer_amd.bispectrum_triangles(n, edges)
    rng = np.random.default_rng(3)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        try:
            full = run_bispectrum(s, d, n, angle, edges, "all")
            assert np.array_equal(full["triples"], every)
            assert np.array_equal(np.rint(full["triangles"]).astype(np.int64), exact)
            assert np.array_equal(np.isnan(full["b"]), exact == 0)
            scale = np.abs(ref["sums"]).max()
            assert np.abs(full["sums"] - ref["sums"]).max() <= 1e-9 * scale
            pick17 = np.sort(rng.choice(5984, 17, replace=False))
            repeats = np.array([100, 7, 100, 5983, 7, 100, 0, 3000, 3000])  # unsorted, with repeats
            for pick in ([2345], pick17, repeats):
                part = run_bispectrum(s, d, n, angle, edges, every[pick])
                for key in ("b", "sums", "triangles"):
                    assert np.array_equal(bits(part[key]), bits(full[key][pick])), (len(pick), key)
        finally:
            s.free(d)


@pytest.mark.gpu
def test_input_off_the_16_byte_grid():
    n, angle = 49, 5.0
    kappa = maps_for(n)[1]
    edges = log_edges(n)
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(kappa)
        padded = s.to_device(np.concatenate([np.zeros(1, np.float32), kappa.ravel(), np.zeros(3, np.float32)]))
        try:
            a = run_bispectrum(s, d, n, angle, edges, "all", maps=True)
            b = run_bispectrum(s, padded + 4, n, angle, edges, "all", maps=True)
        finally:
            s.free(d)
            s.free(padded)
    for key in ("b", "sums", "triangles", "spectrum", "F"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key


@pytest.mark.gpu
def test_run_kappa_equals_run_on_the_read_map():
    n, angle = 64, 3.0
    rng = np.random.default_rng(5)
    planes = (rng.gamma(0.5, 2.0, (3, n, n)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-4, 1e-3, (2, 3))
    with slicer_amd.Slicer(0) as s:
        ptrs = [s.to_device(m) for m in planes]
        try:
            with slicer_amd.Kappa(s, n, 2) as k, slicer_amd.Bispectrum(s, n, angle, edges=log_edges(n)) as b:
                k.add_device(ptrs, coeff.T)
                k.finalize()
                b.run_kappa(k, 1)
                a = b.read()
                d = s.to_device(k.read(1))
                try:
                    b.run(d)
                    again = b.read()
                finally:
                    s.free(d)
                for key in ("b", "sums", "triangles"):
                    assert np.array_equal(bits(a[key]), bits(again[key])), key
                assert set(a) == {"b", "triangles", "sums", "triples", "ell_mean", "counts"}
                bins = slicer_amd.power_bins(n, log_edges(n))
                assert np.array_equal(a["counts"], bins["counts"])
                assert np.array_equal(a["ell_mean"], bins["mean_radius"] * slicer_amd.ell_fundamental(angle), equal_nan=True)
        finally:
            for d in ptrs:
                s.free(d)


@pytest.mark.gpu
def test_bispectrum_errors():
    with slicer_amd.Slicer(0) as s:
        def refused(code, *args, **kw):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Bispectrum(s, *args, **kw)
            assert e.value.code == code, (args, kw)
            return str(e.value)
        e4 = [0.0, 2.0, 4.0, 6.0]
        for n in (37, 44, 0, 1, 16385):
            assert "npix" in refused(6, n, 5.0, edges=e4)  # SLICER_ERR_UNSUPPORTED
        assert "bins" in refused(6, 64, 5.0, edges=np.arange(34.0))  # 33 bins
        assert "bins" in refused(6, 64, 5.0)  # the default edges: 63 bins
        for edges in ([0.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("inf")], [0.0, float("nan")]):
            refused(2, 16, 5.0, edges=edges)  # SLICER_ERR_ARG
        for t in ([1, 0, 2], [0, 2, 1], [-1, 0, 1], [0, 1, 3]):
            assert "triple" in refused(2, 16, 5.0, edges=e4, triples=[t])
        for angle in (0.0, -1.0, float("inf"), float("nan")):
            assert "angle" in refused(2, 16, angle, edges=e4)
        with slicer_amd.Bispectrum(s, 16, 5.0, edges=e4) as b:
            assert b.triangles().shape == (10,)  # readable right after create
            for call in (b.read, b.spectrum, lambda: b.read_map(0)):
                with pytest.raises(slicer_amd.SlicerError) as e:
                    call()
                assert e.value.code == 3  # SLICER_ERR_STATE: nothing has run
            with pytest.raises(slicer_amd.SlicerError) as e:
                b.run(None)
            assert e.value.code == 2
            d = s.to_device(maps_for(16)[0])
            try:
                b.run(d)
                b.read_map(2)
                for k in (-1, 3):
                    with pytest.raises(slicer_amd.SlicerError) as e:
                        b.read_map(k)
                    assert e.value.code == 2
            finally:
                s.free(d)


@pytest.mark.gpu
def test_bispectrum_kernels_are_profiled():
    n = 30
    with slicer_amd.Slicer(0) as s:
        d = s.to_device(maps_for(n)[0])
        try:
            with slicer_amd.Bispectrum(s, n, 5.0, edges=log_edges(n)) as b:
                s.profile_enable(True)
                s.profile_reset()
                b.run(d)
                b.read()
                prof = s.profile_get()
                s.profile_enable(False)
        finally:
            s.free(d)
    for name in ("bispectrum_fft", "bispectrum_band", "bispectrum", "bispectrum_finish"):
        assert name in prof and prof[name][0] == 1, (name, prof)
