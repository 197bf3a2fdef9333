"""Device E/B pseudo-C_l of masked shear maps (slicer_pcl2_*, slicer_amd.PclShear) against the f64
numpy restatement in tests/pcl_shear_np.py, and bit for bit against the scalar pseudo-C_l handle (row N17)."""
import ctypes as C

import numpy as np
import pytest

import pcl_np
import pcl_shear_np
import power_np
import shear_np
import slicer_amd
from test_gpu_pcl import ANGLE, CASES, MASKS as PCL_MASKS, Session, holes, unit_edges
from test_gpu_power import bits, log_edges, maps_for
from test_pcl_shear_host import chiral

MASKS = dict(PCL_MASKS, chiral=lambda n: (chiral(n), 0.0))
NAMES2, NAMES3 = ("EE", "EB", "BE", "BB"), ("EE", "EB", "BE", "BB", "kE", "kB", "Ek", "Bk", "kk")
MATS = ("M0", "M2", "X2", "M4", "X4")
# The bound on M_2, X_2, M_4, X_4: C_M2 * 1e-12 * log2(n) * mean(w^2), row N17's form.  There is no derivation of the
# constant for five chained transforms; it is 8 times the largest max |dev - ref| / (1e-12 log2 n mean w^2) measured
# over test_coupling_matrices' 56 cases and the two grid-stride sizes on an MI355X: 1.376e-4 (n = 30, the taper alone,
# log edges, M_2; per matrix M_2 1.376e-4, M_4 1.374e-4, X_2 6.53e-5, X_4 3.05e-5; n = 16 against the brute-force sums
# gave 9.64e-5 at most, n = 1029 2.05e-5).
C_M2 = 8 * 1.376e-4


def m_bound(n, w):
    return C_M2 * 1e-12 * np.log2(n) * float(np.mean(np.asarray(w, np.float64) ** 2))


def fields_for(n, F, kappa=True):
    """F fields (gamma1, gamma2[, kappa]) of unrelated maps, every map with its own factor."""
    nc = 3 if kappa else 2
    maps = [m * np.float32(0.5 + 0.173 * k) for k, m in enumerate(maps_for(n, F * nc))]
    return [maps[f * nc:(f + 1) * nc] for f in range(F)]


def flat(fields):
    return [m for fld in fields for m in fld]


def set_mask(ss, p, user, width):
    p.set_mask(None if user is None else ss.dev(user), width)


def everything(p, fields_idx):
    """All a handle gives after a run, for bitwise comparisons."""
    r, cp = p.read(), p.coupling()
    out = {"mask": p.mask(), "ell": r["ell"], "counts": r["counts"]}
    out.update({"cl_" + k: v for k, v in r["cl"].items()})
    out.update({"ct_" + k: v for k, v in r["coupled"].items()})
    out.update({k: cp[k] for k in MATS})
    for f in fields_idx:
        for c in range(p.n_comp):
            out[f"sp{f}{c}"] = p.spectrum(f, c).view(np.float64)
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_exact_pins_and_binning(n, split):
    F = 2
    fields = fields_for(n, F)
    user, width = MASKS["taper_holes"](n)
    edges = log_edges(n)
    with Session(split) as ss:
        d = [ss.dev(m) for m in flat(fields)]
        with slicer_amd.Pcl(ss.s, n, ANGLE, 3 * F, cross=True, edges=edges) as q:
            set_mask(ss, q, user, width)
            q.run(d)
            ref = q.read()
            ref_M, ref_w = q.coupling()["M"], q.mask()
            ref_sp = [q.spectrum(k) for k in range(3 * F)]
        got = {}
        for cross in (True, False):
            with slicer_amd.PclShear(ss.s, n, ANGLE, F, with_kappa=True, cross=cross, edges=edges) as p:
                set_mask(ss, p, user, width)
                p.run(d)
                idx = range(F) if cross else [F - 1]
                got[cross] = everything(p, idx)
                set_mask(ss, p, user, width)  # a second round: the same bits everywhere
                p.run(d)
                same_bits(everything(p, idx), got[cross])
        for cross in (True, False):
            g = got[cross]
            assert np.array_equal(g["mask"].view(np.uint32), ref_w.view(np.uint32))
            assert np.array_equal(bits(g["M0"]), bits(ref_M))
            assert np.array_equal(g["counts"], ref["counts"]) and np.array_equal(bits(g["ell"]), bits(ref["ell"]))
            for f in (range(F) if cross else [F - 1]):
                e, b = pcl_shear_np.rotate(ref_sp[3 * f], ref_sp[3 * f + 1])
                assert np.array_equal(g[f"sp{f}0"], e.view(np.float64)), f
                assert np.array_equal(g[f"sp{f}1"], b.view(np.float64)), f
                assert np.array_equal(g[f"sp{f}2"], ref_sp[3 * f + 2].view(np.float64)), f
            for f in range(F):
                for h in (range(F) if cross else [f]):
                    at = (f, h) if cross else (f,)
                    assert np.array_equal(bits(g["ct_kk"][at]), bits(ref["coupled"][3 * f + 2, 3 * h + 2]))
        # auto mode is the diagonal of cross mode
        for k in NAMES3:
            for f in range(F):
                assert np.array_equal(bits(got[False]["ct_" + k][f]), bits(got[True]["ct_" + k][f, f])), (k, f)
        # the binning against the restatement's binning of the handle's own spectra
        g = got[True]
        sp = [g[f"sp{f}{c}"].view(np.complex128) for f in range(F) for c in range(3)]
        pr = power_np.power_of_spectra(sp, ANGLE, edges, cross=True)
        nz = pr["counts"] > 0
        for a, la in enumerate("EBk"):
            for b, lb in enumerate("EBk"):
                for f in range(F):
                    for h in range(F):
                        v = g["ct_" + la + lb][f, h]
                        assert np.array_equal(np.isnan(v), ~nz)
                        err = np.abs(v - pr["cl"][3 * f + a, 3 * h + b])[nz]
                        assert np.all(err <= 1e-13 * pr["scale"][3 * f + a, 3 * h + b][nz]), (la, lb, f, h)


def check_matrices(n, cp, w_ref, edges, label, brute=False):
    ref = pcl_shear_np.matrices(w_ref, edges, brute=brute)
    unit = m_bound(n, w_ref) / C_M2
    worst = 0.0
    for k in MATS[1:]:
        err = float(np.abs(cp[k] - ref[k]).max())
        worst = max(worst, err / unit)
        print(f"{label} {k}: max|dev - ref| / (1e-12 log2 n mean w^2) = {err / unit:.4g}")
    assert worst <= C_M2, worst
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(MASKS))
@pytest.mark.parametrize("n,split", CASES)
def test_coupling_matrices(n, split, kind):
    user, width = MASKS[kind](n)
    w_ref = pcl_np.mask(n, width, user)
    with Session(split) as ss:
        for name, edges in (("log", log_edges(n)), ("unit", unit_edges(n))):
            with slicer_amd.PclShear(ss.s, n, ANGLE, 1, edges=edges) as p:
                set_mask(ss, p, user, width)
                assert np.array_equal(p.mask().view(np.uint32), w_ref.view(np.uint32))
                cp = p.coupling()
            ref = check_matrices(n, cp, w_ref, edges, f"n={n} split={split} mask={kind} edges={name}", brute=n == 16)
            if kind == "chiral":
                assert np.abs(ref["X4"]).max() > 1e-4 and np.abs(ref["X2"]).max() > 1e-4
            act = power_np.binned_sums(n, edges)[0] > 0
            for k in MATS:
                assert not cp[k][~act].any() and not cp[k][:, ~act].any()


def check_decoupling(r, cp, cross, tol, ref=None):
    """read's cl against the block solves of `cp`'s matrices on r's (or ref's) coupled values, within
    tol * cond * max |coupled| of each system's rows; the NaN pattern is the empty bins."""
    act = r["counts"] > 0
    ix = np.flatnonzero(act)
    B = len(act)
    want = ref["cl"] if ref else pcl_shear_np.decouple(cp, r["coupled"], r["counts"], cross)
    src = ref["coupled"] if ref else r["coupled"]
    s4, s2 = pcl_shear_np.system4(cp["M0"], cp["M4"], cp["X4"]), pcl_shear_np.system2(cp["M2"], cp["X2"])

    def cond(system, m):
        idx = np.concatenate([k * B + ix for k in range(m)])
        return np.linalg.cond(system[np.ix_(idx, idx)])
    groups = [(NAMES2, cond(s4, 4))]
    if "kk" in r["cl"]:
        groups += [(("kE", "kB"), cond(s2, 2)), (("Ek", "Bk"), cond(s2, 2)), (("kk",), cond(cp["M0"], 1))]
    F = r["cl"]["EE"].shape[0]
    for names, cnd in groups:
        for f in range(F):
            for g in (range(F) if cross else [f]):
                at = (f, g) if cross else (f,)
                scale = max(np.abs(src[k][at][act]).max() for k in names)
                for k in names:
                    v = r["cl"][k][at]
                    assert np.array_equal(np.isnan(v), ~act), (k, at)
                    assert np.array_equal(np.isnan(r["coupled"][k][at]), ~act), (k, at)
                    err = np.abs(v - want[k][at])[act].max()
                    assert err <= tol * cnd * scale, (k, at, err / (cnd * scale))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(MASKS))
@pytest.mark.parametrize("n,split", CASES)
def test_decoupling(n, split, kind):
    user, width = MASKS[kind](n)
    with Session(split) as ss:
        d3 = [ss.dev(m) for m in flat(fields_for(n, 2))]
        for edges in (log_edges(n), unit_edges(n)):
            for cross, kappa in ((False, True), (True, True), (True, False)):
                d = d3 if kappa else [d3[0], d3[1], d3[3], d3[4]]
                with slicer_amd.PclShear(ss.s, n, ANGLE, 2, with_kappa=kappa, cross=cross, edges=edges) as p:
                    set_mask(ss, p, user, width)
                    p.run(d)
                    r, cp = p.read(), p.coupling()
                assert set(r["cl"]) == set(NAMES3 if kappa else NAMES2)
                check_decoupling(r, cp, cross, 1e-13)


@pytest.mark.gpu
def test_the_whole_chain_recovers_the_restatement():
    """Two fields with kappa, cross mode, the chiral mask: the matrices and the coupled bandpowers within their bounds
    carry over to the solves within cond times their relative errors."""
    n = 45
    user, width = MASKS["chiral"](n)
    fields = fields_for(n, 2)
    edges = unit_edges(n)
    ref = pcl_shear_np.pcl_shear(fields, pcl_np.mask(n, width, user), ANGLE, edges, cross=True)
    with Session(False) as ss, slicer_amd.PclShear(ss.s, n, ANGLE, 2, with_kappa=True, cross=True, edges=edges) as p:
        set_mask(ss, p, user, width)
        p.run([ss.dev(m) for m in flat(fields)])
        r = p.read()
    assert np.array_equal(r["counts"], ref["counts"])
    check_decoupling(r, ref["matrices"], True, 1e-11, ref=ref)


@pytest.mark.gpu
def test_pure_e_without_a_mask():
    """w = 1 at an odd n (no Nyquist lines): the shear of a kappa map is pure E with C_EE = C_kk, bin by bin, the DC bin
    left out (N6 zeroes k = 0 and the rotation is the identity there).

    The bound is N6's, propagated as test_gpu_power.check propagates its spectrum bound: a coefficient of the device's
    kappa spectrum is within eps_k = 1e-12 log2(n) ||kappa||_2 of the exact one, and the f32 maps gamma1, gamma2 the
    handle is given are within N6's output bound 2^-23 |gamma| + 1e-9 max |gamma| of the exact ones pixel by pixel,
    so a coefficient of their transforms is within the sum of that over the pixels (+ eps_k for the device transform,
    ||gamma_i||_2 <= ||kappa||_2); |c2|, |s2| <= 1, so Ehat and Bhat are within the two maps' sums of the exact khat and
    of 0.  With eps = those sums + 3 eps_k (the third for Power's own spectrum, which C_EE is compared with), per mode
    | |Ehat|^2 - |khat|^2 | <= 2 |khat| eps + eps^2 and |Bhat|^2 <= eps^2 (the same bound is asserted for BB and EB)."""
    n = 45
    kappa = shear_np.clustered(n, 2100) + np.float32(0.01)
    edges = unit_edges(n)
    with Session(False) as ss:
        dk = ss.dev(kappa)
        with slicer_amd.Shear(ss.s, n, ANGLE) as sh, slicer_amd.Power(ss.s, n, ANGLE, 1, edges=edges) as pw, \
                slicer_amd.PclShear(ss.s, n, ANGLE, 1, edges=edges) as p:
            sh.run(dk)
            p.set_mask(ss.dev(np.ones((n, n), np.float32)), 0.0)
            p.run_shear([sh])
            r = p.read()
            pw.run([dk])
            ckk = pw.read()["cl"][0]
    exact = shear_np.shear(kappa, ANGLE)
    eps_k = 1e-12 * np.log2(n) * np.linalg.norm(kappa.astype(np.float64))
    eps = 3 * eps_k + sum(float(np.sum(2.0 ** -23 * np.abs(exact[k]) + 1e-9 * np.abs(exact[k]).max()))
                          for k in ("gamma1", "gamma2"))
    counts, (mag,) = power_np.binned_sums(n, edges, [np.abs(exact["spectrum"])])
    theta = np.radians(ANGLE)
    norm = theta * theta / float(n) ** 4
    nz = counts > 0
    nz[0] = False  # the DC bin
    bound = norm * (2 * eps * mag[nz] / counts[nz] + eps * eps) + 1e-13 * np.abs(ckk[nz])
    ee, bb, eb = (r["coupled"][k][0][nz] for k in ("EE", "BB", "EB"))
    print(f"max |EE - kk| / bound = {float((np.abs(ee - ckk[nz]) / bound).max()):.4g}, "
          f"max BB / bound = {float((bb / bound).max()):.4g}, max BB / EE = {float((bb / ee).max()):.4g}")
    assert np.all(np.abs(ee - ckk[nz]) <= bound)
    assert np.all(np.abs(bb) <= bound) and np.all(np.abs(eb) <= bound)
    assert r["coupled"]["EE"][0][0] != ckk[0]  # the mean of kappa is in C_kk's DC bin and not in EE's


@pytest.mark.gpu
@pytest.mark.parametrize("n", [270, 1029])
def test_kernels_past_one_block_and_one_element_a_thread(n):
    """The element-wise kernels run at most 1024 workgroups of 256 threads over the n (n / 2 + 1) half plane: 144
    workgroups with a ragged last one at 270, and two or three elements a thread at 1029.  The phase tables and the
    rotation are checked bitwise through the rotated spectra, the weight spectra and the combination through the
    matrices."""
    H = n // 2 + 1
    assert (256 < n * H < 1024 * 256) if n == 270 else (2 * 1024 * 256 < n * H < 3 * 1024 * 256)
    edges = np.array([0.0, 8.0, float(n // 2)])
    fields = fields_for(n, 1, kappa=False)
    user, width = MASKS["taper_holes"](n)
    w_ref = pcl_np.mask(n, width, user)
    with Session(False) as ss:
        d = [ss.dev(m) for m in fields[0]]
        with slicer_amd.Pcl(ss.s, n, ANGLE, 2, cross=True, edges=edges) as q:
            set_mask(ss, q, user, width)
            q.run(d)
            g = [q.spectrum(k) for k in range(2)]
        with slicer_amd.PclShear(ss.s, n, ANGLE, 1, edges=edges) as p:
            set_mask(ss, p, user, width)
            p.run(d)
            cp, sp = p.coupling(), [p.spectrum(0, c) for c in range(2)]
    e, b = pcl_shear_np.rotate(g[0], g[1])
    assert np.array_equal(bits(sp[0]), bits(e)) and np.array_equal(bits(sp[1]), bits(b))
    check_matrices(n, cp, w_ref, edges, f"n={n}")


def _code(call):
    with pytest.raises(slicer_amd.SlicerError) as e:
        call()
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_pcl_shear_errors():
    n = 16
    L = slicer_amd._lib.load()
    edges = log_edges(n)
    with Session(False) as ss:
        s = ss.s
        for bad_n in (37, 0, 16385):
            assert _code(lambda: slicer_amd.PclShear(s, bad_n, ANGLE, 1, edges=edges))[0] == 6  # SLICER_ERR_UNSUPPORTED
        for nf, kappa in ((0, False), (65, False), (43, True)):
            assert _code(lambda: slicer_amd.PclShear(s, n, ANGLE, nf, with_kappa=kappa, edges=edges))[0] == 6
        for nf, kappa in ((64, False), (42, True)):
            slicer_amd.PclShear(s, n, ANGLE, nf, with_kappa=kappa, edges=edges).close()
        code, text = _code(lambda: slicer_amd.PclShear(s, n, ANGLE, 1, edges=np.arange(130) * 0.05))  # 129 bins
        assert code == 6 and "at most 128" in text
        for e in ([0.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("nan")]):
            assert _code(lambda: slicer_amd.PclShear(s, n, ANGLE, 1, edges=e))[0] == 2  # SLICER_ERR_ARG
        for angle in (0.0, float("inf")):
            assert _code(lambda: slicer_amd.PclShear(s, n, angle, 1, edges=edges))[0] == 2
        ph = C.c_void_p()
        assert L.slicer_pcl2_create(s._h, n, ANGLE, 1, 0, 0, n, None, C.byref(ph)) == 2  # the edges are required
        e = np.ascontiguousarray(edges)
        assert L.slicer_pcl2_create(s._h, n, ANGLE, 1, 2, 0, e.size, e.ctypes.data, C.byref(ph)) == 2
        assert L.slicer_pcl2_create(s._h, n, ANGLE, 1, 0, 2, e.size, e.ctypes.data, C.byref(ph)) == 2
        assert "slicer_pcl2_create" in _code(lambda: slicer_amd.PclShear(s, 37, ANGLE, 1, edges=edges))[1]
        with pytest.raises(ValueError):
            slicer_amd.PclShear(s, n, ANGLE, 1)

        d = [ss.dev(m) for m in flat(fields_for(n, 2))]
        good = ss.dev(holes(n))
        with slicer_amd.PclShear(s, n, ANGLE, 2, with_kappa=True, edges=edges) as p:
            def usable():
                p.set_mask(good, 3.0)
                assert _code(p.read)[0] == 3  # a new mask invalidates the last run
                p.run(d)
                r = p.read()
                assert all(np.all(np.isfinite(v[:, r["counts"] > 0])) for v in r["cl"].values())
            # before a mask / before a run: SLICER_ERR_STATE
            for call in (lambda: p.run(d), p.coupling, p.mask, p.read, lambda: p.spectrum(1, 0)):
                assert _code(call)[0] == 3
            usable()
            nan = np.ones((n, n), np.float32)
            nan[3, 5] = np.nan
            inf = np.ones((n, n), np.float32)
            inf[0, 0] = np.inf
            refusals = [lambda: p.set_mask(None, 0.0), lambda: p.set_mask(good, -1.0),
                        lambda: p.set_mask(good, float("nan")), lambda: p.set_mask(good, float("inf")),
                        lambda: p.set_mask(ss.dev(nan), 0.0), lambda: p.set_mask(ss.dev(inf), 3.0),
                        lambda: p.set_mask(ss.dev(np.zeros((n, n), np.float32)), 0.0),
                        lambda: p.set_mask(ss.dev(np.zeros((n, n), np.float32)), 3.0)]
            for k, call in enumerate(refusals):
                code, text = _code(call)
                assert code == 2, k
                if k in (4, 5):
                    assert "slicer_pcl2_set_mask" in text and "not finite" in text
                if k >= 6:
                    assert "coupling matrix singular" in text
                if k >= 4:  # refused after the arguments: the handle has no mask now
                    assert _code(p.mask)[0] == 3 and _code(lambda: p.run(d))[0] == 3
                usable()
            assert _code(lambda: p.run(d[:5] + [0]))[0] == 2
            with pytest.raises(ValueError):
                p.run(d[:4])
            assert _code(lambda: p.spectrum(2, 0))[0] == 2 and _code(lambda: p.spectrum(-1, 0))[0] == 2
            assert _code(lambda: p.spectrum(1, 3))[0] == 2
            assert _code(lambda: p.spectrum(0, 0))[0] == 3  # auto mode keeps only the last field's spectra
            p.spectrum(1, 2)
            usable()
        with slicer_amd.PclShear(s, n, ANGLE, 1, edges=edges) as p:
            p.set_mask(good, 0.0)
            p.run(d[:2])
            assert _code(lambda: p.spectrum(0, 2))[0] == 2  # no kappa in this handle
            assert set(p.read()["cl"]) == set(NAMES2)
