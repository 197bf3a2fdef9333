"""Device wavelet scattering coefficients (slicer_scattering_*, slicer_amd.Scattering) against the
numpy restatement of tests/scattering_np.py, which takes the direct complex ifft2 where the device takes the Hermitian
split through two real inverses.

The bound, per coefficient: 16 x 0.14 U + 64 * 2^-52 |value|, U = 2^-52 log2(n) sqrt(mean kappa^2); per pixel of a
modulus field the same with U on max |kappa| (scattering_np.device_bound).  Every test prints its largest error as a
fraction of the bound.  Largest values measured on an MI355X over all cases: s1 0.031, p1 0.029, s2 0.017, first-order
fields 0.032, second-order fields 0.008 of the bound.

Sizes named from the constants of slicer_scattering.hip: 1024^2 has 128 chunks of kMinChunk = 8192 pixels, 128 values a
lane, two rounds of the kInner = 64 block loop of k_scat_sums, and 1024 * 513 half-plane modes, more than the
8 * 256 * 256 threads one round of k_scat_filter has on 256 compute units.  96^2, 105^2 and 128^2 have two chunks, the
second ragged at 105^2; every smaller size has one, ragged against the wave where n^2 is no multiple of 64."""
import math

import numpy as np
import pytest

import scattering_np as SN
import slicer_amd
import stream_util

ARG, STATE, UNSUPPORTED = 2, 3, 6
SIZES = [12, 15, 16, 21, 30, 49, 64, 96, 105, 128]
INPUTS = {"white": SN.white, "lognormal": SN.lognormal}


def banks_of(n):
    return [(1, 1), (1, 4), (2, 3), (3, 4), (int(math.floor(math.log2(n))), 2), (2, 16)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("s0", "s1", "p1", "s2"))


def worst_ratios(got, ref, kappa):
    """The largest error of s1, p1 and s2 as a fraction of the bound, after checking s0 and the NaN pattern."""
    u = SN.unit(kappa)
    assert np.all(np.abs(got["s0"] - ref["s0"]) <= SN.device_bound(ref["s0"], u))
    m = np.isfinite(ref["s2"])
    assert np.array_equal(np.isnan(got["s2"]), ~m)
    out = {}
    for key in ("s1", "p1"):
        out[key] = float((np.abs(got[key] - ref[key]) / SN.device_bound(ref[key], u)).max())
    out["s2"] = float((np.abs(got["s2"] - ref["s2"])[m] / SN.device_bound(ref["s2"][m], u)).max()) if m.any() else 0.0
    return out


def inside(r, what):
    print(what, "error / bound:", {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, (what, r)


def field_ratio(got, ref, kappa):
    return float((np.abs(got - ref) / SN.device_bound(ref, SN.unit(kappa, per_pixel=True))).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(INPUTS))
@pytest.mark.parametrize("n", SIZES)
def test_against_the_restatement(n, kind):
    kappa = INPUTS[kind](n, 100 + n)
    with stream_util.Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, kappa)
        for J, L in banks_of(n):
            ref = SN.coefficients(kappa, J, L)
            with slicer_amd.Scattering(S, n, J, L) as x:
                x.run(d)
                got = x.read()
                assert got["s1"].shape == (J, L) and got["s2"].shape == (J, L, J, L)
                x.run(d)
                assert same_bits(x.read(), got)
            assert np.all(got["s1"] > 0) and np.all(got["p1"] >= got["s1"] ** 2 * (1 - 1e-12))
            inside(worst_ratios(got, ref, kappa), f"n = {n}, {kind}, J = {J}, L = {L}:")
        assert np.array_equal(S.to_host(d, (n, n), np.float32), kappa)  # the input is only read


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 16, 105])
def test_modulus_fields_per_pixel(n):
    J, L = 3, 3
    kappa = SN.lognormal(n, 7)
    k64 = kappa.astype(np.float64)
    worst = {"first": 0.0, "second": 0.0}
    with stream_util.Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, kappa)
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        x.run(d)
        before = x.read()
        for j1, l1 in [(0, 0), (1, 2), (2, 1)]:
            u1 = SN.modulus(k64, SN.filter_bank(n, J, L, j1, l1))
            got = x.modulus(d, j1, l1)
            assert got.shape == (n, n)
            worst["first"] = max(worst["first"], field_ratio(got, u1, kappa))
            # the field's mean is the coefficient, to the rounding of another summation order: no running sum of the
            # device's is longer than 64 terms, then 2 blocks, 6 butterfly steps and 2 chunks, all of one sign
            assert abs(got.mean() - before["s1"][j1, l1]) <= 64 * SN.EPS * before["s1"][j1, l1]
            for j2, l2 in [(j1 + 1, 0), (J - 1, 2)]:
                if j2 <= j1 or j2 >= J:
                    continue
                u2 = SN.modulus(u1, SN.filter_bank(n, J, L, j2, l2))
                got2 = x.modulus(d, j1, l1, j2, l2)
                worst["second"] = max(worst["second"], field_ratio(got2, u2, kappa))
                assert abs(got2.mean() - before["s2"][j1, l1, j2, l2]) <= 64 * SN.EPS * before["s2"][j1, l1, j2, l2]
        assert same_bits(x.read(), before)  # modulus leaves the last run's results readable
        for bad in [(-1, 0, -1, -1), (J, 0, -1, -1), (0, L, -1, -1), (1, 0, 1, 0), (1, 0, 0, 0), (0, 0, J, 0), (0, 0, 1, L),
                    (0, 0, 1, -1), (0, 0, -1, 0)]:
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.modulus(d, *bad)
            assert e.value.code == ARG and "slicer_scattering_modulus" in str(e.value)
    inside(worst, f"n = {n}: modulus fields,")


@pytest.mark.gpu
def test_planted_inputs():
    n, J, L = 64, 3, 4
    with stream_util.Scope() as sc:
        S = sc.slicer()
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        # a constant map: nothing but the mean
        const = np.full((n, n), 0.37, np.float32)
        x.run(sc.device(S, const))
        r = x.read()
        u = SN.unit(const)
        m = np.isfinite(r["s2"])
        assert abs(r["s0"][0] - float(const[0, 0])) <= 4 * SN.EPS and abs(r["s0"][1] - float(const[0, 0]) ** 2) <= 4 * SN.EPS
        assert float(np.abs(r["s1"]).max()) <= SN.DEVICE_U * u and float(np.abs(r["s2"][m]).max()) <= SN.DEVICE_U * u
        assert float(np.abs(r["p1"]).max()) <= SN.DEVICE_U * u
        print("constant map: largest |s1|, |s2| in U:", float(np.abs(r["s1"]).max()) / u, float(np.abs(r["s2"][m]).max()) / u)
        # one pixel: u1 is the modulus of the filter in real space, moved to the pixel
        spike = np.zeros((n, n), np.float32)
        spike[5, 9] = 2.0
        d = sc.device(S, spike)
        x.run(d)
        r = x.read()
        worst = 0.0
        for j in range(J):
            for l in range(L):
                psi = np.roll(2.0 * np.abs(np.fft.ifft2(SN.filter_bank(n, J, L, j, l))), (5, 9), (0, 1))
                worst = max(worst, field_ratio(x.modulus(d, j, l), psi, spike))
                assert abs(r["s1"][j, l] - psi.mean()) <= SN.device_bound(psi.mean(), SN.unit(spike))
        inside({"fields": worst}, "single pixel:")
        # one plane wave at the peak of psi^_{1,0}: xi n / (2 pi) = 3 n / 16 = 12 along axis 0
        a0 = 12
        wave = np.cos(2.0 * np.pi * a0 * np.arange(n) / n)[:, None].repeat(n, 1).astype(np.float32)
        x.run(sc.device(S, wave))
        r = x.read()
        ref = SN.coefficients(wave, J, L)
        inside(worst_ratios(r, ref, wave), "plane wave:")
        psi = SN.filter_bank(n, J, L, 1, 0)
        assert np.unravel_index(np.argmax(psi), psi.shape) == (a0, 0)
        # u1 = |c+ e^(i phi) + c- e^(-i phi)| = |c+| |1 + q e^(-2 i phi)|, q = psi^[-a0] / psi^[a0] (about -0.03: beta B^
        # at -xi): its mean is |c+| (1 + q^2 / 4 + ...), it leaves that mean by |q| |c+| at most, no filter exceeds 2,
        # and the roundings of the f32 wave add about 2^-24 of other harmonics
        leak = abs(psi[n - a0, 0] / psi[a0, 0]) + 2.0 ** -20
        assert leak < 0.05
        s1 = r["s1"][1, 0]
        assert abs(s1 - psi[a0, 0] / 2.0) <= leak * leak * s1
        assert np.all(r["s2"][1, 0, 2] <= 2.0 * leak * s1 + SN.device_bound(0.0, SN.unit(wave)))
        print("plane wave: s1 =", s1, "largest s2 / s1 =", float(r["s2"][1, 0, 2].max()) / s1)


@pytest.mark.gpu
def test_roll_and_transpose_relations_on_the_device():
    n, J, L = 21, 3, 4
    kappa = SN.lognormal(n, 8)
    u = SN.unit(kappa)
    perm = (L // 2 - np.arange(L)) % L
    with stream_util.Scope() as sc:
        S = sc.slicer()
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        reads = []
        for k in (kappa, np.roll(kappa, (4, -7), (0, 1)), np.ascontiguousarray(kappa.T)):
            x.run(sc.device(S, k))
            reads.append(x.read())
    base, rolled, tr = reads
    m = np.isfinite(base["s2"])
    want = {"s1": base["s1"][:, perm], "p1": base["p1"][:, perm], "s2": base["s2"][:, perm][:, :, :, perm]}
    for key in ("s1", "p1", "s2"):  # two device results, each within the bound of the truth
        mk = m if key == "s2" else np.ones(base[key].shape, bool)
        assert np.all(np.abs(rolled[key] - base[key])[mk] <= 2 * SN.device_bound(base[key][mk], u)), key
        assert np.all(np.abs(tr[key] - want[key])[mk] <= 2 * SN.device_bound(want[key][mk], u)), key
    assert float(np.abs(tr["s1"] - base["s1"]).max()) > 1e6 * u  # the permutation is not the identity


@pytest.mark.gpu
def test_bitwise_repeatable_second_map_and_unaligned_pointer():
    n, J, L = 49, 3, 3
    a, b = SN.lognormal(n, 9), SN.white(n, 10)
    with stream_util.Scope() as sc:
        S = sc.slicer()
        da, db = sc.device(S, a), sc.device(S, b)
        shifted = sc.device(S, np.concatenate([np.zeros(1, np.float32), a.ravel()]))  # a, one float off the 16-byte grid
        assert da % 16 == 0 and shifted % 16 == 0
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        x.run(da)
        ra = x.read()
        x.run(db)
        rb = x.read()
        inside(worst_ratios(rb, SN.coefficients(b, J, L), b), "a second map on the same handle:")
        assert not same_bits(ra, rb)
        x.run(da)
        assert same_bits(x.read(), ra)
        x.run(shifted + 4)
        assert same_bits(x.read(), ra)
        assert np.array_equal(bits(x.modulus(shifted + 4, 1, 1, 2, 0)), bits(x.modulus(da, 1, 1, 2, 0)))
        with slicer_amd.Scattering(S, n, J, L) as y:  # a fresh handle gives the same bits
            y.run(da)
            assert same_bits(y.read(), ra)
        assert np.array_equal(S.to_host(da, (n, n), np.float32), a)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [30, 105, 128])
def test_both_shear_split_settings_are_inside_the_bound(n):
    J, L = 3, 2
    kappa = SN.lognormal(n, 11)
    ref = SN.coefficients(kappa, J, L)
    with stream_util.Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, kappa)
        for split in (0, 1):
            S.set_option("shear_split", split)
            try:
                with slicer_amd.Scattering(S, n, J, L) as x:
                    x.run(d)
                    inside(worst_ratios(x.read(), ref, kappa), f"n = {n}, shear_split = {split}:")
            finally:
                S.set_option("shear_split", 0)


@pytest.mark.gpu
def test_run_on_a_user_stream():
    n, J, L = 30, 2, 3
    kappa = SN.white(n, 12)
    with stream_util.Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, kappa)
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        x.run(d)
        own, field = x.read(), x.modulus(d, 0, 1)
        inside(worst_ratios(own, SN.coefficients(kappa, J, L), kappa), "the handle's own stream:")
        st = sc.stream(nonblocking=True)
        S.set_stream(st.ptr)
        x.run(d)
        assert same_bits(x.read(), own)
        assert np.array_equal(bits(x.modulus(d, 0, 1)), bits(field))
        S.set_stream(None)


@pytest.mark.gpu
def test_read_before_run_and_the_create_refusals():
    with stream_util.Scope() as sc:
        S = sc.slicer()
        x = sc.sub(slicer_amd.Scattering(S, 16, 2, 2))
        with pytest.raises(slicer_amd.SlicerError) as e:
            x.read()
        assert e.value.code == STATE and "slicer_scattering_read before any slicer_scattering_run" in str(e.value)
        with pytest.raises(slicer_amd.SlicerError) as e:
            x.run(None)
        assert e.value.code == ARG
        for npix, J, L, code, text in [(22, 2, 2, UNSUPPORTED, "npix = 22 unsupported"), (16, 13, 2, UNSUPPORTED, "J = 13 above 12"),
                                       (16, 2, 17, UNSUPPORTED, "L = 17 above 16"), (16, 0, 2, ARG, "J = 0 below 1"),
                                       (16, 2, 0, ARG, "L = 0 below 1"), (16, 5, 2, ARG, "2^J = 32 above npix = 16")]:
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Scattering(S, npix, J, L)
            assert e.value.code == code and "slicer_scattering_create: " + text in str(e.value)


@pytest.mark.gpu
def test_one_large_map_and_the_profile_names():
    """1024^2: the block loop of k_scat_sums past one round, k_scat_filter past one grid-stride round."""
    n, J, L = 1024, 3, 2
    kappa = SN.lognormal(n, 13)
    ref = SN.coefficients(kappa, J, L)
    with stream_util.Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, kappa)
        x = sc.sub(slicer_amd.Scattering(S, n, J, L))
        S.profile_enable(True)
        S.profile_reset()
        x.run(d)
        got = x.read()
        prof = S.profile_get()
        S.profile_enable(False)
        inside(worst_ratios(got, ref, kappa), "1024^2:")
        # one scope for khat and s0 and one per (j1, l1); one second-order scope per (j1, l1) that has a j2 above it
        assert prof["scattering_first"][0] == 1 + J * L and prof["scattering_second"][0] == (J - 1) * L
        j1, l1, j2, l2 = 0, 1, 2, 0
        u1 = SN.modulus(kappa.astype(np.float64), SN.filter_bank(n, J, L, j1, l1))
        u2 = SN.modulus(u1, SN.filter_bank(n, J, L, j2, l2))
        inside({"first": field_ratio(x.modulus(d, j1, l1), u1, kappa),
                "second": field_ratio(x.modulus(d, j1, l1, j2, l2), u2, kappa)}, "1024^2 modulus fields:")
