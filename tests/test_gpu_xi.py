"""Device real-space two-point functions (slicer_xi_*, slicer_amd.Xi) against the direct pair sums
of tests/xi_np.py, one lag at a time, shared through tests/xi_cases.py.

The bound: 16 times the reference figure REF_U = 0.36 U_b, the numpy FFT route against the same direct sums (re-measured
by tests/test_xi_host.py), U_b = 2^-52 log2(P) M_b norm / W_b (xi_np.unit).  Every test prints the largest device error
in units of U_b.  Largest values measured on an MI355X over all cases: W_b 1.0 U,
xi 0.421 U, xi+- 0.606 U, single lags of the window 0.331 U.

Cases named from the constants of slicer_xi.hip: (40, 32) has a lag window of 2 L + 1 = 65 columns, one more than the
kXiCols = 64 of one k_xi_bin workgroup, so a second workgroup per bin holds a single column ((96, 40) and (97, 23) have a
ragged second chunk, (33, 31) stays one column below); (40, 30) with 300 bins has more sums than the kSumThreads = 256 of
one k_xi_sum workgroup."""
import math

import numpy as np
import pytest

import slicer_amd
import xi_cases
import xi_np

ARG, STATE, UNSUPPORTED = 2, 3, 6
PARAMS = [(n, L, P, bins, split, kind) for (n, L, P, bins) in xi_cases.CASES for split in (0, 1)
          for kind in xi_cases.WEIGHTS]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Session:
    """A Slicer with shear_split set, and the device copies it made."""

    def __init__(self, split):
        self.s = slicer_amd.Slicer(0)
        self.s.set_option("shear_split", int(split))
        self.ptrs = []

    def dev(self, a):
        self.ptrs.append(self.s.to_device(np.ascontiguousarray(a, np.float32)))
        return self.ptrs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.s.free(p)
        self.s.set_option("shear_split", 0)
        self.s.close()


def run_twice(x, ptrs):
    """read() of a run, after checking that a second run gives the same bits."""
    x.run(ptrs)
    r = x.read()
    x.run(ptrs)
    again = x.read()
    for k in r:
        if r[k].dtype == np.float64:
            assert np.array_equal(bits(again[k]), bits(r[k])), k
        else:
            assert np.array_equal(again[k], r[k]), k
    return r


def check_geometry(r, d):
    """counts, W_b, r_mean and the NaN pattern; returns the W_b error in units of U."""
    live = d.live()
    assert np.array_equal(r["counts"], d.N)
    worst = 0.0
    if d.w is None:
        assert np.array_equal(r["weights"], d.N.astype(np.float64))
    else:
        u = xi_np.unit(d.P, d.M, d.sumw2)
        has = d.M > 0
        err = np.abs(r["weights"] - d.Wb)[has] / u[has]
        worst = float(err.max())
        assert worst <= xi_cases.DEVICE_U
        assert np.all(r["weights"][~has] == 0.0)
    assert np.array_equal(np.isnan(r["r"]), ~live)
    assert np.all(np.abs(r["r"][live] - d.r[live]) <= 1e-12 * d.r[live])
    return worst


def check_xi(got, ref, u, live, what):
    assert np.array_equal(np.isnan(got), ~live), what
    err = float((np.abs(got - ref)[live] / u[live]).max())
    assert err <= xi_cases.DEVICE_U, (what, err)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("n,L,P,bins,split,kind", PARAMS)
def test_against_direct_sum(n, L, P, bins, split, kind):
    d = xi_cases.direct(n, L, bins, kind)
    maps = xi_cases.maps_for(n)
    live = d.live()
    assert live.any() and (~live).any()
    if kind == "corner":  # bins with lags but no pair of non-zero weight: NaN; the inner ones are right
        assert ((d.M > 0) & ~live).any()
    worst = {"W": 0.0, "xi": 0.0, "xipm": 0.0}
    with Session(split) as ss:
        dm = [ss.dev(m) for m in maps]
        dw = None if d.w is None else ss.dev(d.w)
        F0, F2 = xi_cases.SPIN0, xi_cases.SPIN2
        auto = {}
        with slicer_amd.Xi(ss.s, n, 0, 3, d.edges) as x:
            assert x.max_lag == L
            if kind != "none":  # without a call the handle has w = 1
                x.set_weights(dw)
            r = run_twice(x, [dm[i] for i in F0])
            worst["W"] = check_geometry(r, d)
            for f, i in enumerate(F0):
                ref, u = d.spin0(i, i)
                worst["xi"] = max(worst["xi"], check_xi(r["xi"][f], ref, u, live, ("auto", i)))
                auto[i] = r["xi"][f]
        with slicer_amd.Xi(ss.s, n, 0, 3, d.edges, cross=True) as x:
            x.set_weights(dw)
            r = run_twice(x, [dm[i] for i in F0])
            check_geometry(r, d)
            for s, t in xi_cases.pairs(3):
                ref, u = d.spin0(F0[s], F0[t])
                worst["xi"] = max(worst["xi"], check_xi(r["xi"][s, t], ref, u, live, ("cross", s, t)))
            for f, i in enumerate(F0):  # the same field alone or among all pairs: the same bits
                assert np.array_equal(bits(r["xi"][f, f]), bits(auto[i]))
        with slicer_amd.Xi(ss.s, n, 2, 1, d.edges) as x:
            x.set_weights(dw)
            r = run_twice(x, [dm[F2[0][0]], dm[F2[0][1]]])
            check_geometry(r, d)
            rp, rm, u = d.spin2(F2[0], F2[0])
            worst["xipm"] = max(worst["xipm"], check_xi(r["xip"][0], rp, u, live, "xi+"),
                                check_xi(r["xim"][0], rm, u, live, "xi-"))
            one = r
        with slicer_amd.Xi(ss.s, n, 2, 2, d.edges, cross=True) as x:
            x.set_weights(dw)
            r = run_twice(x, [dm[i] for f in F2 for i in f])
            check_geometry(r, d)
            for s, t in xi_cases.pairs(2):
                rp, rm, u = d.spin2(F2[s], F2[t])
                worst["xipm"] = max(worst["xipm"], check_xi(r["xip"][s, t], rp, u, live, ("xi+", s, t)),
                                    check_xi(r["xim"][s, t], rm, u, live, ("xi-", s, t)))
            assert np.array_equal(bits(r["xip"][0, 0]), bits(one["xip"][0]))
            assert np.array_equal(bits(r["xim"][0, 0]), bits(one["xim"][0]))
    print(f"n={n} L={L} P={P} B={len(d.edges) - 1} split={split} w={kind}: W_b {worst['W']:.3g} U, "
          f"xi {worst['xi']:.3g} U, xi+- {worst['xipm']:.3g} U (bound {xi_cases.DEVICE_U:.3g} U)")


@pytest.mark.gpu
@pytest.mark.parametrize("n,L,P,bins,split,kind", [p for p in PARAMS if p[3] == 0 and p[5] in ("none", "binary")])
def test_lag_windows(n, L, P, bins, split, kind):
    """slicer_xi_correlation against the per-lag direct sums.  Every spectrum is real, so an inverse is the part of its
    correlation that is even in r."""
    d = xi_cases.direct(n, L, bins, kind)
    maps = xi_cases.maps_for(n)
    even = lambda win: 0.5 * (win + xi_np.flip(win))
    eps = xi_cases.DEVICE_U * 2.0 ** -52 * math.log2(P)  # U of one lag, before the norm
    worst = 0.0
    with Session(split) as ss:
        dm = [ss.dev(m) for m in maps]
        dw = None if d.w is None else ss.dev(d.w)
        F0, F2 = xi_cases.SPIN0, xi_cases.SPIN2
        with slicer_amd.Xi(ss.s, n, 0, 3, d.edges, cross=True) as x:
            x.set_weights(dw)
            got = x.correlation(0, slicer_amd.XI_WEIGHTS)  # before any run
            if d.w is None:
                assert np.array_equal(got, d.Wwin)
            else:
                err = float(np.abs(got - d.Wwin).max()) / (eps * d.sumw2)
                worst = max(worst, err)
                assert err <= 1.0
            x.run([dm[i] for i in F0])
            for p, (s, t) in enumerate(xi_cases.pairs(3)):
                got = x.correlation(p)
                norm = math.sqrt(d.norm[F0[s]] * d.norm[F0[t]])
                err = float(np.abs(got - even(d.C(F0[s], F0[t]))).max()) / (eps * norm)
                worst = max(worst, err)
                assert err <= 1.0, (s, t)
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.correlation(0, slicer_amd.XI_MINUS)
            assert e.value.code == ARG
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.correlation(6)
            assert e.value.code == ARG
        with slicer_amd.Xi(ss.s, n, 2, 2, d.edges, cross=True) as x:
            x.set_weights(dw)
            x.run([dm[i] for f in F2 for i in f])
            for p, (s, t) in enumerate(xi_cases.pairs(2)):
                a, b = F2[s], F2[t]
                ref = xi_np.spin2_windows(d.C(a[0], b[0]), d.C(a[1], b[1]), d.C(a[0], b[1]), d.C(a[1], b[0]))
                norm = math.sqrt((d.norm[a[0]] + d.norm[a[1]]) * (d.norm[b[0]] + d.norm[b[1]]))
                for which in (slicer_amd.XI_PLUS, slicer_amd.XI_MINUS, slicer_amd.XI_CROSS):
                    err = float(np.abs(x.correlation(p, which) - even(ref[which])).max()) / (eps * norm)
                    worst = max(worst, err)
                    assert err <= 1.0, (s, t, which)
        with slicer_amd.Xi(ss.s, n, 0, 2, d.edges) as x:  # auto mode keeps the last field's transform only
            x.run([dm[0], dm[1]])
            err = float(np.abs(x.correlation(1) - d.C(1, 1)).max()) / (eps * d.norm[1]) if d.w is None else 0.0
            assert err <= 1.0
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.correlation(0)
            assert e.value.code == STATE
    print(f"n={n} L={L} P={P} split={split} w={kind}: lag windows at most {worst * xi_cases.DEVICE_U:.3g} U of one lag")


@pytest.mark.gpu
def test_refusals():
    n, edges = 12, [0.0, 2.0, 5.0]
    with Session(0) as ss:
        s = ss.s
        for spin in (1, -2, 4):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Xi(s, n, spin, 1, edges)
            assert e.value.code == ARG and "spin" in str(e.value)
        for nf, code in ((0, ARG), (-1, ARG), (33, UNSUPPORTED)):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Xi(s, n, 0, nf, edges)
            assert e.value.code == code and "n_fields" in str(e.value)
        with pytest.raises(slicer_amd.SlicerError) as e:
            slicer_amd.Xi(s, 9000, 0, 1, [0.0, 8999.0])
        assert e.value.code == UNSUPPORTED and "no transform size up to 16384" in str(e.value)
        for bad, code in (([0.0, 16.0], ARG), ([0.0, 2.0, 2.0], ARG), ([0.0, float("nan")], ARG), ([3.0], ARG)):
            with pytest.raises(slicer_amd.SlicerError) as e:
                slicer_amd.Xi(s, n, 0, 1, bad)
            assert e.value.code == code
        m = ss.dev(xi_cases.maps_for(n)[0])
        with slicer_amd.Xi(s, n, 0, 1, edges) as x:
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.read()
            assert e.value.code == STATE and "before any slicer_xi_run" in str(e.value)
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.correlation(0)
            assert e.value.code == STATE
            for v in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
                w = np.ones((n, n), np.float32)
                w[7, 3] = v
                with pytest.raises(slicer_amd.SlicerError) as e:
                    x.set_weights(ss.dev(w))
                assert e.value.code == ARG and "1 values that are negative or not finite" in str(e.value)
                with pytest.raises(slicer_amd.SlicerError) as e:  # no weights any more
                    x.run([m])
                assert e.value.code == STATE
            x.set_weights(None)
            x.run([m])
            x.read()
            x.set_weights(ss.dev(np.ones((n, n), np.float32)))  # new weights invalidate the run
            with pytest.raises(slicer_amd.SlicerError) as e:
                x.read()
            assert e.value.code == STATE
            with pytest.raises(ValueError):
                x.run([m, m])
        with slicer_amd.Xi(s, n, 2, 1, edges) as x:
            with pytest.raises(ValueError):
                x.run([m])
            x.run([m, m])
            assert set(x.read()) >= {"xip", "xim"}


@pytest.mark.gpu
def test_unsupported_map_size_works():
    """n itself need not be a size the transform plans: n = 97 is prime (above); here n = 4004 = 4 * 7 * 11 * 13 at a small
    window."""
    n, edges = 4004, np.array([0.5, 1.2, 1.5, 2.0])
    assert not slicer_amd.shear_supported(n)
    rng = np.random.default_rng(5)
    a = (1.0 + rng.standard_normal((n, n))).astype(np.float32)
    f = a.astype(np.float64)
    L = 2
    win = xi_np.window(f, f, L)
    N, M = xi_np.enumerate_bins(n, edges)
    ref = xi_np.bin_sum(win, n, edges) / N
    with Session(0) as ss:
        with slicer_amd.Xi(ss.s, n, 0, 1, edges) as x:
            x.run([ss.dev(a)])
            r = x.read()
    P = xi_np.padded_size(n, L)
    assert P == 4032
    u = xi_np.unit(P, M, float(np.sum(f * f)), N.astype(np.float64))
    assert np.array_equal(r["counts"], N)
    err = float((np.abs(r["xi"][0] - ref) / u).max())
    print(f"n={n} P={P}: xi {err:.3g} U")
    assert err <= xi_cases.DEVICE_U
