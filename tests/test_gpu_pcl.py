"""Device masked pseudo-C_l (slicer_pcl_*, slicer_amd.Pcl) against the f64 numpy restatement in
tests/pcl_np.py, and bit for bit against the shear and power handles on the host-multiplied maps."""
import ctypes as C

import numpy as np
import pytest

import pcl_np
import slicer_amd
from test_gpu_power import bits, log_edges, maps_for, run_power, shear_spectrum

ANGLE = 5.0
CASES = [(n, False) for n in (16, 30, 45, 49, 128)] + [(30, True), (128, True)]
# The bound on M: C_M * 1e-12 * log2(n) * mean(w^2), the form of the spectrum bound of row N6.  There is no derivation
# of the constant for three chained transforms; it is 8 times the largest max |M_dev - M_ref| / (1e-12 log2 n mean w^2)
# measured over test_coupling_matrix's 42 cases on an MI355X: 1.473e-4 (n = 49, the taper times three holes, log edges;
# n = 16 against the brute-force sum gave 8.0e-5 at most).
C_M = 8 * 1.473e-4


def unit_edges(n):
    return np.arange(n // 2 + 1, dtype=np.float64)


def holes(n):
    """Three rectangular holes."""
    u = np.ones((n, n), np.float32)
    u[n // 5:n // 5 + max(2, n // 8), n // 4:n // 4 + max(3, n // 6)] = 0.0
    u[n // 2:n // 2 + max(1, n // 10), n // 2 + 1:n // 2 + 1 + max(2, n // 7)] = 0.0
    u[(3 * n) // 4:(3 * n) // 4 + 2, n // 8:n // 8 + max(2, n // 5)] = 0.0
    return u


def binary(n):
    return (np.random.default_rng(77 + n).random((n, n)) < 0.7).astype(np.float32)


MASKS = {"taper": lambda n: (None, n / 5.0), "taper_holes": lambda n: (holes(n), n / 5.0),
         "binary": lambda n: (binary(n), 0.0)}


def m_bound(n, w):
    return C_M * 1e-12 * np.log2(n) * float(np.mean(np.asarray(w, np.float64) ** 2))


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


def set_mask(ss, p, user, width):
    p.set_mask(None if user is None else ss.dev(user), width)


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_exact_pins(n, split):
    maps = maps_for(n, 3)
    user, width = MASKS["taper_holes"](n)
    edges = log_edges(n)
    f = slicer_amd.pcl_taper(n, width)
    with Session(split) as ss:
        d = [ss.dev(m) for m in maps]
        got = {}
        for cross in (False, True):
            with slicer_amd.Pcl(ss.s, n, ANGLE, 3, cross=cross, edges=edges) as p:
                set_mask(ss, p, user, width)
                w = p.mask()
                assert np.array_equal(w.view(np.uint32), ((f[:, None] * f[None, :]).astype(np.float32) * user).view(np.uint32))
                p.run(d)
                r = p.read()
                M = p.coupling()["M"]
                r["spectra"] = {k: p.spectrum(k) for k in (range(3) if cross else [2])}
                set_mask(ss, p, user, width)  # a second round: bitwise the same M and cl
                p.run(d)
                assert np.array_equal(bits(p.coupling()["M"]), bits(M))
                again = p.read()
                assert np.array_equal(bits(again["cl"]), bits(r["cl"]))
                assert np.array_equal(bits(again["coupled"]), bits(r["coupled"]))
                got[cross] = r
        pre = [w * m for m in maps]  # the host products, f32
        for cross in (False, True):
            ref = run_power(ss.s, pre, ANGLE, cross, edges, split)
            ss.s.set_option("shear_split", int(split))  # run_power resets it
            r = got[cross]
            assert np.array_equal(bits(r["coupled"]), bits(ref["cl"]))
            assert np.array_equal(r["counts"], ref["counts"])
            assert np.array_equal(bits(r["ell"]), bits(ref["ell"]))
        for k in range(3):
            sp = shear_spectrum(ss.s, pre[k], ANGLE, split)
            ss.s.set_option("shear_split", int(split))
            assert np.array_equal(bits(got[True]["spectra"][k]), bits(sp)), k
        assert np.array_equal(bits(got[False]["spectra"][2]), bits(got[True]["spectra"][2]))


@pytest.mark.gpu
@pytest.mark.parametrize("n,split", CASES)
def test_constant_masks(n, split):
    # White-noise maps, auto spectra: the bound on cl is relative to every bandpower by itself, and the rounding of M's
    # off-diagonal elements (some 1e-16) leaks every bin's power into every other bin, so the bound can only hold where
    # the bandpowers of one spectrum are within a few decades of each other.
    maps = maps_for(n, 3)[::2]
    with Session(split) as ss:
        d = [ss.dev(m) for m in maps]
        for edges in (log_edges(n), unit_edges(n)):
            B = len(edges) - 1
            raw = run_power(ss.s, maps, ANGLE, False, edges, split)
            ss.s.set_option("shear_split", int(split))
            act = raw["counts"] > 0
            eye = np.diag(act.astype(np.float64))
            with slicer_amd.Pcl(ss.s, n, ANGLE, 2, edges=edges) as p:
                for c in (1.0, 0.5):
                    w = np.full((n, n), c, np.float32)
                    set_mask(ss, p, w, 0.0)
                    cp = p.coupling()
                    assert cp["M"].shape == (B, B)
                    err = float(np.abs(cp["M"] - c * c * eye).max())
                    print(f"n={n} split={split} c={c} B={B}: |M - c^2 I| / unit = {err / (m_bound(n, w) / C_M):.4g}")
                    assert err <= m_bound(n, w)
                    assert cp["mean_w"] == c and cp["mean_w2"] == c * c
                    if c == 1.0:
                        p.run(d)
                        r = p.read()
                        assert np.array_equal(np.isnan(r["cl"]), np.isnan(raw["cl"]))
                        rel = np.abs(r["cl"] - raw["cl"])[..., act] / np.abs(raw["cl"][..., act])
                        print(f"n={n} split={split} B={B}: max |cl - cl_raw| / |cl_raw| = {float(rel.max()):.4g}")
                        assert np.all(rel <= 1e-12)


@pytest.mark.gpu
def test_dc_bin_is_kept():
    """r_0 = 0 and w = 1: the first bin of log_edges holds m2 = 0 alone, and M[0][0] = 1 only if the band indicator
    keeps that mode."""
    n = 16
    with Session(False) as ss, slicer_amd.Pcl(ss.s, n, ANGLE, 1, edges=log_edges(n)) as p:
        w = np.ones((n, n), np.float32)
        set_mask(ss, p, w, 0.0)
        assert slicer_amd.power_bins(n, log_edges(n))["counts"][0] == 1
        assert abs(p.coupling()["M"][0, 0] - 1.0) <= m_bound(n, w)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [270, 1029])
def test_mask_kernels_past_one_pixel_a_thread(n):
    """k_pcl_moments is 256 workgroups of 256 threads, k_pcl_mask at most 4096: a thread takes a second pixel from n^2 >
    65536 and n^2 > 2^20 on, and CASES stop at 128 (where three quarters of the moments' workgroups have no pixel).  270
    and 1029 are the smallest sizes the transform takes past 256 and 1024; both leave the last round ragged."""
    assert 256 * 256 < 270 * 270 < 2 * 256 * 256 and 4096 * 256 < 1029 * 1029 < 2 * 4096 * 256
    N = float(n * n)
    edges = np.array([0.0, 8.0, float(n // 2)])
    with Session(False) as ss, slicer_amd.Pcl(ss.s, n, ANGLE, 1, edges=edges) as p:
        user, width = MASKS["taper_holes"](n)
        w_ref = pcl_np.mask(n, width, user)
        set_mask(ss, p, user, width)
        assert np.array_equal(p.mask().view(np.uint32), w_ref.view(np.uint32))
        cp, w64 = p.coupling(), w_ref.astype(np.float64)
        # the moments: the bound of test_coupling_matrix
        assert abs(cp["mean_w"] - w64.mean()) <= 2 * N * 2.0 ** -53 * w64.mean()
        assert abs(cp["mean_w2"] - (w64 ** 2).mean()) <= 2 * N * 2.0 ** -53 * (w64 ** 2).mean()
        # zeros and ones: every partial sum is an integer, so a pixel dropped or taken twice changes the means exactly
        user = binary(n)
        set_mask(ss, p, user, 0.0)
        assert np.array_equal(p.mask().view(np.uint32), user.view(np.uint32))
        cp = p.coupling()
        assert cp["mean_w"] == cp["mean_w2"] == float(user.sum(dtype=np.int64)) / N
        # values that are not finite are counted in every round: a thread's second pixel, and the map's last one
        bad = user.copy().ravel()
        bad[[256 * 256 + 5, n * n - 1]] = np.nan, np.inf
        code, text = _code(lambda: set_mask(ss, p, bad.reshape(n, n), 0.0))
        assert code == 2 and "2 values that are not finite" in text


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(MASKS))
@pytest.mark.parametrize("n,split", CASES)
def test_coupling_matrix(n, split, kind):
    user, width = MASKS[kind](n)
    w_ref = pcl_np.mask(n, width, user)
    N = float(n * n)
    with Session(split) as ss:
        for name, edges in (("log", log_edges(n)), ("unit", unit_edges(n))):
            ref = pcl_np.coupling_brute(w_ref, edges) if n == 16 else pcl_np.coupling_fft(w_ref, edges)
            with slicer_amd.Pcl(ss.s, n, ANGLE, 1, edges=edges) as p:
                set_mask(ss, p, user, width)
                assert np.array_equal(p.mask().view(np.uint32), w_ref.view(np.uint32))
                cp = p.coupling()
            # the moments: sums of n^2 positive f64 terms, each sum within (n^2 - 1) 2^-53 of the exact one
            w64 = w_ref.astype(np.float64)
            assert abs(cp["mean_w"] - w64.mean()) <= 2 * N * 2.0 ** -53 * w64.mean()
            assert abs(cp["mean_w2"] - (w64 ** 2).mean()) <= 2 * N * 2.0 ** -53 * (w64 ** 2).mean()
            err = float(np.abs(cp["M"] - ref).max())
            print(f"n={n} split={split} mask={kind} edges={name}: max|M_dev - M_ref| / (1e-12 log2 n mean w^2) = "
                  f"{err / (m_bound(n, w_ref) / C_M):.4g}")
            assert err <= m_bound(n, w_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [30, 45])
def test_split_chains_at_both_parities(n):
    """shear_split = 1 at 30 (rows in 2 passes, columns in 3) and at 45 (3 and 3: every pass buffer of the plan is in
    use; odd, so the rows are loaded and stored as packed pairs and the last pair lacks its second row).  CASES has no odd
    size under shear_split, and this handle is the only one behind the masked row load and the |khat|^2 column load.
    The masked transform has the bits of the plain one of the f32 products (Pcl.spectrum against Power.spectrum), and M
    is inside test_coupling_matrix's bound of numpy's f64 rfft2 / irfft2 route."""
    maps = maps_for(n, 3)
    user, width = MASKS["taper_holes"](n)
    w_ref = pcl_np.mask(n, width, user)
    edges = log_edges(n)
    with Session(True) as ss:
        d = [ss.dev(m) for m in maps]
        with slicer_amd.Pcl(ss.s, n, ANGLE, 3, cross=True, edges=edges) as p:
            set_mask(ss, p, user, width)
            assert np.array_equal(p.mask().view(np.uint32), w_ref.view(np.uint32))
            M = p.coupling()["M"]
            p.run(d)
            spectra = [p.spectrum(k) for k in range(3)]
        err = float(np.abs(M - pcl_np.coupling_fft(w_ref, edges)).max())
        print(f"n={n} split: max|M_dev - M_ref| / (1e-12 log2 n mean w^2) = {err / (m_bound(n, w_ref) / C_M):.4g}")
        assert err <= m_bound(n, w_ref)
        ref = run_power(ss.s, [w_ref * m for m in maps], ANGLE, True, edges, True)
        for k in range(3):
            assert np.array_equal(bits(spectra[k]), bits(ref["spectra"][k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(MASKS))
@pytest.mark.parametrize("n,split", CASES)
def test_decoupling(n, split, kind):
    user, width = MASKS[kind](n)
    maps = maps_for(n, 2)
    with Session(split) as ss:
        d = [ss.dev(m) for m in maps]
        for edges in (log_edges(n), unit_edges(n)):
            for cross in (False, True):
                with slicer_amd.Pcl(ss.s, n, ANGLE, 2, cross=cross, edges=edges) as p:
                    set_mask(ss, p, user, width)
                    p.run(d)
                    r, M = p.read(), p.coupling()["M"]
                act = r["counts"] > 0
                assert np.array_equal(np.isnan(r["cl"]), np.broadcast_to(~act, r["cl"].shape))
                assert np.array_equal(np.isnan(r["coupled"]), np.broadcast_to(~act, r["cl"].shape))
                Ma = M[np.ix_(act, act)]
                cond = np.linalg.cond(Ma)
                flat, cflat = r["cl"].reshape(-1, len(act)), r["coupled"].reshape(-1, len(act))
                for q in range(flat.shape[0]):
                    ref = np.linalg.solve(Ma, cflat[q, act])
                    bound = 1e-13 * cond * np.abs(cflat[q, act]).max()
                    assert np.all(np.abs(flat[q, act] - ref) <= bound), (cross, q, cond)


@pytest.mark.gpu
def test_decoupling_recovers_the_restatement():
    """The whole chain against the restatement from the maps and the mask: M and the coupled bandpowers within their
    bounds carry over to the solve within cond(M) times their relative errors."""
    n = 45
    user, width = MASKS["taper_holes"](n)
    maps = maps_for(n, 2)
    edges = unit_edges(n)
    ref = pcl_np.pcl(maps, pcl_np.mask(n, width, user), ANGLE, edges, cross=True)
    with Session(False) as ss, slicer_amd.Pcl(ss.s, n, ANGLE, 2, cross=True, edges=edges) as p:
        set_mask(ss, p, user, width)
        p.run([ss.dev(m) for m in maps])
        r = p.read()
    act = ref["counts"] > 0
    cond = np.linalg.cond(ref["M"][np.ix_(act, act)])
    scale = np.abs(ref["cl"][..., act]).max()
    assert np.all(np.abs(r["cl"] - ref["cl"])[..., act] <= 1e-11 * cond * scale)


@pytest.mark.gpu
def test_run_kappa_and_ell_edges():
    n, angle = 32, 3.0
    rng = np.random.default_rng(5)
    planes = (rng.gamma(0.5, 2.0, (3, n, n)) * 3.0).astype(np.float32)
    coeff = rng.uniform(1e-4, 1e-3, (2, 3))
    ell_edges = unit_edges(n) * slicer_amd.ell_fundamental(angle)
    with Session(False) as ss:
        ptrs = [ss.dev(m) for m in planes]
        with slicer_amd.Kappa(ss.s, n, 2) as k, slicer_amd.Pcl(ss.s, n, angle, 2, ell_edges=ell_edges) as p:
            k.add_device(ptrs, coeff.T)
            k.finalize()
            p.set_mask(None, 4.0)
            p.run_kappa(k)
            a = p.read()
            p.run([ss.dev(k.read(i)) for i in range(2)])
            b = p.read()
            assert np.array_equal(bits(a["cl"]), bits(b["cl"]))
            assert np.array_equal(a["counts"], slicer_amd.power_bins(n, p.edges)["counts"])


def _code(call):
    with pytest.raises(slicer_amd.SlicerError) as e:
        call()
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_pcl_errors():
    n = 16
    L = slicer_amd._lib.load()
    edges = log_edges(n)
    with Session(False) as ss:
        s = ss.s
        for bad_n in (37, 0, 16385):
            assert _code(lambda: slicer_amd.Pcl(s, bad_n, ANGLE, 1, edges=edges))[0] == 6  # SLICER_ERR_UNSUPPORTED
        for nm in (0, 129):
            assert _code(lambda: slicer_amd.Pcl(s, n, ANGLE, nm, edges=edges))[0] == 6
        assert _code(lambda: slicer_amd.Pcl(s, n, ANGLE, 1, edges=np.arange(514) * 0.01))[0] == 6  # 513 bins
        for e in ([0.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("nan")]):
            assert _code(lambda: slicer_amd.Pcl(s, n, ANGLE, 1, edges=e))[0] == 2  # SLICER_ERR_ARG
        for angle in (0.0, float("inf")):
            assert _code(lambda: slicer_amd.Pcl(s, n, angle, 1, edges=edges))[0] == 2
        ph = C.c_void_p()
        assert L.slicer_pcl_create(s._h, n, ANGLE, 1, 0, n, None, C.byref(ph)) == 2  # the edges are required
        with pytest.raises(ValueError):
            slicer_amd.Pcl(s, n, ANGLE, 1)

        maps = maps_for(n, 2)
        d = [ss.dev(m) for m in maps]
        good = ss.dev(holes(n))
        with slicer_amd.Pcl(s, n, ANGLE, 2, edges=edges) as p:
            def usable():
                p.set_mask(good, 3.0)
                assert _code(p.read)[0] == 3  # a new mask invalidates the last run
                p.run(d)
                assert np.all(np.isfinite(p.read()["cl"][:, p.read()["counts"] > 0]))
            # before a mask / before a run: SLICER_ERR_STATE
            for call in (lambda: p.run(d), p.coupling, p.mask, p.read, lambda: p.spectrum(1)):
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
                if k >= 6:
                    assert "coupling matrix singular" in text
                usable()
            assert _code(lambda: p.run([d[0], 0]))[0] == 2
            assert _code(lambda: p.spectrum(2))[0] == 2
            assert _code(lambda: p.spectrum(0))[0] == 3  # auto mode keeps only the last map's spectrum
            p.spectrum(1)
            usable()
