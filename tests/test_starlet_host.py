"""The restatement tests/starlet_np.py of slicer_starlet_* and slicer_l1norm_*  against a plain loop
over Python floats, the properties that follow from the definition, slicer_starlet_gains, and every refusal that needs
no device."""
import ctypes as C
import math

import numpy as np
import pytest

import slicer_amd
import starlet_np as W
from slicer_amd import lensing

L = lensing._L
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, 2, 3, 6
MAX = 131072


def _err(h=None):
    return (L.slicer_last_error(h) or b"").decode()


# ---- the restatement against a plain loop ----------------------------------------------------------
def refl_loop(i, n):
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p  # Python's: non-negative
    return m if m < n else p - m


def line_loop(v, n, d, axis):
    """A_d along `axis` of the n x n list of lists of Python floats; every operation one rounded f64 operation."""
    out = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            at = (lambda o: v[refl_loop(i + o, n)][j]) if axis == 0 else (lambda o: v[i][refl_loop(j + o, n)])
            a = at(-d) + at(d)
            b = at(-2 * d) + at(2 * d)
            out[i][j] = (((6.0 * at(0)) + (4.0 * a)) + b) * 0.0625
    return out


def starlet_loop(x, scales):
    n = x.shape[0]
    c = [[float(x[i, j]) for j in range(n)] for i in range(n)]
    w = []
    for s in range(scales):
        d = 1 << s
        c1 = line_loop(line_loop(c, n, d, 1), n, d, 0)
        with np.errstate(invalid="ignore", over="ignore"):
            w.append(np.array([[c[i][j] - c1[i][j] for j in range(n)] for i in range(n)], np.float64).astype(np.float32))
        c = c1
    with np.errstate(invalid="ignore", over="ignore"):
        return [np.array(c, np.float64).reshape(n, n).astype(np.float32)] + w


def same(got, ref):
    """Equal values and equal NaN positions."""
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and bool(
        np.all((got == ref) | (np.isnan(got) & np.isnan(ref))))


def make_map(n, seed=0, special=False):
    rng = np.random.default_rng(1009 * n + seed)
    x = (np.exp(rng.standard_normal((n, n))) - 1.6).astype(np.float32)
    if special:
        flat = x.ravel()
        for k, v in enumerate((np.nan, np.inf, -np.inf)):
            flat[(7 * k + seed) % flat.size] = v
    return x


@pytest.mark.parametrize("n", range(1, 10))
def test_the_restatement_is_the_plain_loop(n):
    for scales in range(1, 6):  # at n = 9 the reach 2 * 16 passes the map four times over
        for special in (False, True):
            x = make_map(n, scales, special)
            got, ref = W.starlet(x, scales), starlet_loop(x, scales)
            assert len(got) == len(ref) == scales + 1
            for s in range(scales + 1):
                assert same(got[s], ref[s]), (n, scales, special, s)


def test_refl_mirrors_without_repeating_the_edge():
    assert W.refl(np.arange(-9, 10), 1).tolist() == [0] * 19
    assert W.refl(np.arange(-5, 9), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert W.refl(np.arange(-3, 5), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    for n in (2, 3, 7):
        for i in range(-40, 40):
            assert int(W.refl(np.array([i]), n)[0]) == refl_loop(i, n)


# ---- what follows from the definition ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_a_constant_map_is_its_own_coarse_map(n):
    for value in (3.25, -1e-3, 1e30, 0.1):
        x = np.full((n, n), value, np.float32)
        out = W.starlet(x, 7)
        assert out[0].tobytes() == x.tobytes()
        assert all(not w.any() for w in out[1:])


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 33, 100, 257])
def test_the_scales_sum_back_to_the_map(n):
    for scales in (1, 3, 6, 9):
        x = make_map(n, scales)
        out = W.starlet(x, scales)
        total = sum(o.astype(np.float64) for o in out)
        bound = 2.0 ** -24 * sum(np.abs(o).astype(np.float64) for o in out) * (1 + 2.0 ** -20)
        assert (np.abs(total - x.astype(np.float64)) <= bound).all(), (n, scales)


def test_a_non_finite_pixel_reaches_the_support_and_nothing_else():
    n, scales = 21, 4
    clean = make_map(n)
    for value in (np.nan, np.inf):
        for at in ((0, 0), (3, 17), (20, 9)):
            x = clean.copy()
            x[at] = value
            out, ref, reach = W.starlet(x, scales), W.starlet(clean, scales), W.reach(x, scales)
            for s in range(scales + 1):
                assert np.array_equal(~np.isfinite(out[s]), reach[s]), (value, at, s)
                assert out[s][~reach[s]].tobytes() == ref[s][~reach[s]].tobytes()
    one = np.zeros((n, n), bool)
    one[10, 10] = True
    x = np.where(one, np.float32(np.nan), clean)
    # scale 1 away from the edges: the 5 x 5 block of c_1 about the pixel
    assert np.argwhere(W.reach(x, 1)[1]).tolist() == [[i, j] for i in range(8, 13) for j in range(8, 13)]


# ---- gains ------------------------------------------------------------------------------------------
def test_gains_are_the_definition_in_long_double():
    for scales in (1, 2, 5, 7):
        got, got_coarse = slicer_amd.starlet_gains(scales)
        ref, ref_coarse = W.gains(scales)
        assert got.shape == (scales,)
        # both are long double sums rounded to f64 at the end: one ulp for the rounding, one for the sums
        assert np.all(np.abs(got - ref.astype(np.float64)) <= 2 * np.spacing(got)), scales
        assert abs(got_coarse - float(ref_coarse)) <= 2 * np.spacing(got_coarse)
    # a longer call starts with the shorter one
    assert slicer_amd.starlet_gains(12)[0][:5].tobytes() == slicer_amd.starlet_gains(5)[0].tobytes()


def test_gains_are_the_published_ones():
    g, _ = slicer_amd.starlet_gains(3)
    assert np.all(np.abs(g - np.array([0.8907963, 0.2006639, 0.0855075])) < 1e-6)


def test_gains_are_the_rms_of_an_impulse_response():
    """White noise of unit variance through a linear map has the variance sum of the squared impulse response."""
    scales = 4
    n = 8 * (1 << scales) + 1
    x = np.zeros((n, n), np.float32)
    x[n // 2, n // 2] = 1.0
    out = W.starlet(x, scales)  # (the taps are dyadic: every c_j here is exact, the outputs are rounded to f32 once)
    g, coarse = slicer_amd.starlet_gains(scales)
    rms = [math.sqrt(float((o.astype(np.float64) ** 2).sum())) for o in out]
    assert np.all(np.abs(np.array(rms[1:]) - g) <= 2.0 ** -23 * g) and abs(rms[0] - coarse) <= 2.0 ** -23 * coarse


# The gains do not square-sum to one: w_i and w_j of one noise map are correlated (neighbouring bands overlap), so the
# variance of their sum, 1, is sum_j gain_j^2 + gain_coarse^2 plus twice the covariances.  Already at J = 1 the identity
# fails: 0.8907963^2 + 0.2734375^2 = 0.868, and the covariance of w_1 and c_1, (6/16)^2 - (70/256)^2 = 0.0659, enters twice.
def test_gains_square_sum_below_one():
    g, coarse = slicer_amd.starlet_gains(1)
    assert coarse == 70.0 / 256.0 and abs(g[0] ** 2 + coarse ** 2 + 2 * (36.0 / 256.0 - coarse ** 2) - 1) < 1e-15
    assert g[0] ** 2 + coarse ** 2 < 0.87


def test_gains_refusals():
    for bad in (0, -1, 13):
        with pytest.raises(slicer_amd.SlicerError) as e:
            slicer_amd.starlet_gains(bad)
        assert e.value.code == ERR_ARG
        assert _err() == f"slicer_starlet_gains: scales = {bad} outside 1..12"
    assert L.slicer_starlet_gains(3, None, None) == OK


# ---- refusals without a device ---------------------------------------------------------------------------
EDGES = np.array([1.0, 3.0, 5.0])
E = EDGES.ctypes.data
BUF = np.zeros(64)
P = BUF.ctypes.data


@pytest.mark.parametrize("null_out", [False, True])
def test_starlet_create_without_a_handle(null_out):
    who = "slicer_starlet_create: "
    cases = [((0, 3), ERR_ARG, who + "npix must be positive"),
             ((MAX + 1, 3), ERR_UNSUPPORTED, who + f"npix = {MAX + 1} above {MAX}"),
             ((16, 0), ERR_ARG, who + "scales = 0 outside 1..12"),
             ((16, 13), ERR_ARG, who + "scales = 13 outside 1..12"),
             ((0, 13), ERR_ARG, who + "npix must be positive"),  # npix is looked at first
             ((16, 12), ERR_ARG, who + "null argument"),
             ((MAX, 1), ERR_ARG, who + "null argument")]
    for args, code, text in cases:
        out = C.c_void_p(1)
        assert L.slicer_starlet_create(None, *args, None if null_out else C.byref(out)) == code, args
        assert _err() == text
        assert out.value == (1 if null_out else None)  # *out is cleared before anything else


@pytest.mark.parametrize("null_out", [False, True])
def test_l1norm_create_without_a_handle_refuses_as_peaks_does(null_out):
    """The same calls to slicer_peaks_create and slicer_l1norm_create: the same codes and, but for the name, texts."""
    nan_edges = np.array([1.0, np.nan, 5.0])
    flat_edges = np.array([1.0, 1.0, 5.0])
    many = np.arange(1026.0)
    calls = [(0, 3, E), (MAX + 1, 3, E), (16, 1, E), (16, 1027, many.ctypes.data), (16, 3, None),
             (16, 3, nan_edges.ctypes.data), (16, 3, flat_edges.ctypes.data), (16, 3, E), (16, 1025, many.ctypes.data),
             (0, 1, None), (16, 1, None)]
    seen = set()
    for args in calls:
        answers = []
        for name in ("peaks", "l1norm"):
            out = C.c_void_p(1)
            code = getattr(L, f"slicer_{name}_create")(None, *args, None if null_out else C.byref(out))
            answers.append((code, _err().replace(f"slicer_{name}_create", "create"), out.value))
        assert answers[0] == answers[1] and answers[0][0] != OK, args
        seen.add(answers[0][:2])
    assert len(seen) == 7 and (ERR_UNSUPPORTED, f"create: npix = {MAX + 1} above {MAX}") in seen


NULL_HANDLE = [
    ("slicer_starlet_run", (P,), "slicer_starlet_run: null argument"),
    ("slicer_starlet_run_npix", (P, 16), "slicer_starlet_run_npix: null argument"),
    ("slicer_starlet_device_map", (0, C.byref(C.c_void_p())), "slicer_starlet_device_map: null argument"),
    ("slicer_starlet_read", (0, P), "slicer_starlet_read: null argument"),
    ("slicer_l1norm_run", (P,), "slicer_l1norm_run: null argument"),
    ("slicer_l1norm_run_npix", (P, 16), "slicer_l1norm_run_npix: null argument"),
    ("slicer_l1norm_read", (P, None, None, None, None, None, None), "slicer_l1norm_read: null handle"),
]


@pytest.mark.parametrize("name,args,text", NULL_HANDLE, ids=[c[0] for c in NULL_HANDLE])
def test_entry_points_without_a_handle(name, args, text):
    assert getattr(L, name)(None, *args) == ERR_ARG
    assert _err() == text


@pytest.mark.parametrize("name", ["starlet", "l1norm"])
def test_destroy_without_a_handle(name):
    L.slicer_power_read(None, None, None, None)  # leaves a text behind: destroy sets none
    assert getattr(L, f"slicer_{name}_destroy")(None) == ERR_ARG
    assert _err() == "slicer_power_read: null handle"


def test_the_l1_restatement_on_a_small_case():
    x = np.array([[0.5, -1.5, 2.0, np.nan], [-3.0, 3.0, np.inf, -np.inf], [1.0, -0.0, 2.5, 0.999], [7.0, -7.0, 1.5, 2.0]],
                 np.float32)
    r = W.l1norm(x, [-3.0, 1.0, 2.0, 3.0])
    # bins [-3, 1), [1, 2), [2, 3]: the last closed; -3 on the first edge is inside
    assert r["counts"].tolist() == [5, 2, 4] and r["below"] == 2 and r["above"] == 2 and r["nan"] == 1
    assert r["l1"].tolist() == [0.5 + 1.5 + 3.0 + 0.0 + float(np.float32(0.999)), 2.5, 9.5]
    assert r["below_l1"] == math.inf and r["above_l1"] == math.inf
    assert W.l1norm(np.float32([[4.0, -9.0]]), [0.0, 1.0])["below_l1"] == 9.0
