"""The moments-over-a-halving-pyramid contract without a device: the restatement
tests/moments_np.py against brute force and against a scalar loop in the order of Lens/halve.py, the emulation of the device's summation order
inside the counted bound with f64 accumulators and outside it with f32 ones, the depth formula, and the refusals of
slicer_moments_* that need no device."""
import ctypes as C

import numpy as np
import pytest

import moments_np as M
import slicer_amd
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6
LD = np.longdouble


def _err():
    return (L.slicer_last_error(None) or b"").decode()


def inputs(n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    g = rng.standard_normal((n, n))
    return {"white": g.astype(np.float32), "lognormal": (np.exp(g) - np.exp(0.5)).astype(np.float32),
            "offset": (1.0 + 1e-3 * g).astype(np.float32)}


@pytest.mark.parametrize("n", range(1, 10))
def test_restatement_against_a_plain_loop(n):
    x = inputs(n)["lognormal"]
    c = np.float64(0.1)
    S = [LD(0)] * 7
    A = [LD(0)] * 7
    tot = LD(0)
    for i in range(n):
        for j in range(n):
            d = LD(x[i, j]) - LD(c)
            tot += LD(x[i, j])
            for k in range(2, 9):
                S[k - 2] += d ** k
                A[k - 2] += abs(d) ** k
    s, a = M.sums_ld(x, c)
    assert np.allclose(np.array(S, LD), s, rtol=1e-17, atol=0) and np.allclose(np.array(A, LD), a, rtol=1e-17, atol=0)
    assert abs(M.mean_ld(x)[0] - tot / n ** 2) <= 1e-18
    for mode in ("sum", "mean"):
        pyr = M.pyramid(x, int(np.log2(n)), mode)
        assert [p.shape[0] for p in pyr] == [n >> l for l in range(len(pyr))]
        for lo, hi in zip(pyr[1:], pyr[:-1]):
            for i in range(lo.shape[0]):
                for j in range(lo.shape[0]):
                    y = np.float32(np.float32(np.float32(hi[2 * i, 2 * j] + hi[2 * i + 1, 2 * j]) + hi[2 * i, 2 * j + 1])
                                   + hi[2 * i + 1, 2 * j + 1])
                    assert lo[i, j] == (np.float32(0.25) * y if mode == "mean" else y)


def test_gaussian_noise_has_gaussian_moments():
    n, sigma = 512, 0.7
    x = (sigma * np.random.default_rng(5).standard_normal((n, n))).astype(np.float32)
    s, _ = M.sums_ld(x, float(M.mean_ld(x)[0]))
    m = (s / LD(n * n)).astype(np.float64)
    N = n * n
    assert abs(m[0] - sigma ** 2) <= 5 * np.sqrt(2.0 / N) * sigma ** 2
    assert abs(m[1]) <= 5 * np.sqrt(15.0 / N) * sigma ** 3
    assert abs(m[2] - 3 * sigma ** 4) <= 5 * np.sqrt(96.0 / N) * sigma ** 4


def halve_scalar_loop(x):
    """The contract's order, one output pixel at a time: the 2x2 block's four f32 scalars added left to right as
    (row 2i, col 2j), (row 2i+1, col 2j), (row 2i, col 2j+1), (row 2i+1, col 2j+1), each partial sum rounded to f32.
    floor(n/2) outputs a side, so an odd map's last row and column stay out."""
    f32 = np.float32
    h = x.shape[0] // 2
    y = np.empty((h, h), f32)
    for out_r in range(h):
        top, bot = x[2 * out_r], x[2 * out_r + 1]
        for out_c in range(h):
            left, right = 2 * out_c, 2 * out_c + 1
            acc = f32(top[left])
            for term in (bot[left], top[right], bot[right]):
                acc = f32(acc + f32(term))
            y[out_r, out_c] = acc
    return y


@pytest.mark.parametrize("n", [4, 5, 10])
def test_halving_order_is_the_one_of_halve_py(n):
    rng = np.random.default_rng(n)
    # mixed magnitudes, so that the order of the three additions shows in the last bits
    x = (rng.standard_normal((n, n)) * 10.0 ** rng.integers(-3, 4, (n, n))).astype(np.float32)
    ref = halve_scalar_loop(x)
    assert np.array_equal(M.halve(x, "sum").view(np.uint32), ref.view(np.uint32))
    h = n // 2
    a, b, c, d = (x[r:2 * h:2, s:2 * h:2] for r, s in ((0, 0), (1, 0), (0, 1), (1, 1)))
    other = (a + c) + (b + d)  # rows first: another order
    assert not np.array_equal(other.view(np.uint32), ref.view(np.uint32))
    assert np.allclose(other, ref, rtol=1e-5)


@pytest.mark.parametrize("n", [7, 64, 257, 1000])
def test_emulation_is_inside_the_bound_with_f64_and_outside_with_f32(n):
    for name, x in inputs(n).items():
        mean, mean_abs = M.mean_ld(x)
        c = np.float64(mean)
        ref, A = M.sums_ld(x, c)
        bound = M.sum_bounds(A, n)
        s64, m64 = M.emulate(x, c, np.float64)
        ratio = np.abs(s64.astype(LD) - ref) / bound
        assert ratio.max() <= 1, (name, ratio)
        assert abs(LD(m64) - mean) <= M.mean_bound(mean_abs, n), name
        s32, m32 = M.emulate(x, c, np.float32)
        ratio32 = np.abs(s32.astype(LD) - ref) / bound
        assert ratio32.max() > 1, (name, ratio32)
        assert abs(LD(m32) - mean) > M.mean_bound(mean_abs, n), name


def test_depth_is_the_formula():
    for n in list(range(1, 200)) + [255, 256, 257, 1000, 1023, 1024, 4095, 4096, 4097, 8192, 16383, 16384, 65536, 131072]:
        assert L.slicer_moments_depth(n) == M.depth(n) == slicer_amd.moments_depth(n), n
    assert M.depth(16384) == 290 <= 8192
    assert M.depth(1) == 8 + 18 + 1
    for bad in (0, -3, 131073):
        assert L.slicer_moments_depth(bad) == -1
        assert _err() == f"slicer_moments_depth: npix = {bad} outside 1..131072"
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.moments_depth(0)


@pytest.mark.parametrize("npix,levels,mode,code,text", [
    (0, 0, 0, ERR_ARG, "npix must be positive"),
    (-4, 0, 0, ERR_ARG, "npix must be positive"),
    (131073, 0, 0, ERR_UNSUPPORTED, "npix = 131073 above 131072"),
    (16, -1, 0, ERR_ARG, "levels = -1 outside 0..4 for npix = 16"),
    (16, 5, 0, ERR_ARG, "levels = 5 outside 0..4 for npix = 16"),
    (31, 5, 1, ERR_ARG, "levels = 5 outside 0..4 for npix = 31"),
    (1, 1, 0, ERR_ARG, "levels = 1 outside 0..0 for npix = 1"),
    (16, 2, 2, ERR_ARG, "mode = 2, expected SLICER_HALVE_MEAN or SLICER_HALVE_SUM"),
    (16, 2, -1, ERR_ARG, "mode = -1, expected SLICER_HALVE_MEAN or SLICER_HALVE_SUM"),
    (16, 4, 1, ERR_ARG, "null argument"),
])
def test_create_refusals_need_no_device(npix, levels, mode, code, text):
    out = C.c_void_p(1)
    assert L.slicer_moments_create(None, npix, levels, mode, C.byref(out)) == code
    assert _err() == "slicer_moments_create: " + text
    assert not out.value
    assert L.slicer_moments_create(None, npix, levels, mode, None) == code


def test_calls_without_a_handle():
    buf = np.zeros(8)
    p = C.c_void_p()
    assert L.slicer_moments_run(None, buf.ctypes.data, None) == ERR_ARG
    assert _err() == "slicer_moments_run: null argument"
    assert L.slicer_moments_read(None, None, buf.ctypes.data, None, None) == ERR_ARG
    assert _err() == "slicer_moments_read: null handle"
    assert L.slicer_moments_device_map(None, 1, C.byref(p)) == ERR_ARG
    assert _err() == "slicer_moments_device_map: null argument"
    assert L.slicer_moments_read_map(None, 1, buf.ctypes.data) == ERR_ARG
    assert _err() == "slicer_moments_read_map: null argument"
    assert L.slicer_moments_destroy(None) == ERR_ARG


def test_python_wrapper_refuses_a_bad_mode_and_an_empty_combination():
    with pytest.raises(ValueError):
        slicer_amd.Moments(None, 16, 0, mode="median")
    with pytest.raises(ValueError):
        slicer_amd.combine_moments([])
