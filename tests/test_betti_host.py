"""The Betti-number contract without a device: the restatement tests/betti_np.py against the
Euler count of the Minkowski restatement (components - holes = vertices - edges + faces, exactly, on every map), its
answers by hand on small shapes, and the refusals of slicer_betti_* that need no device."""
import ctypes as C

import numpy as np
import pytest

import betti_np as BT
import minkowski_np as MK
import slicer_amd
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6


def _err():
    return (L.slicer_last_error(None) or b"").decode()


def make_map(n, kind, seed=0):
    rng = np.random.default_rng(104729 * n + seed)
    if kind == "integers":
        return rng.integers(-3, 4, (n, n)).astype(np.float32)
    g = rng.standard_normal((n, n), np.float32)
    return (g if kind == "white" else np.exp(g) - np.float32(np.exp(0.5))).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 33, 65])
@pytest.mark.parametrize("kind", ["white", "lognormal", "integers"])
def test_components_minus_holes_is_the_euler_count_of_the_pixel_complex(n, kind):
    lo, hi = {"white": (-2.5, 3.0), "lognormal": (-1.25, 6.0), "integers": (-2.0, 2.0)}[kind]
    for seed in range(3):
        x = make_map(n, kind, seed)
        if n >= 7 and seed == 2:
            x[n // 2, n // 3] = np.nan
            x[0, 1] = np.nan
            x[n - 1, n - 2] = -np.inf
            x[2, 2] = np.inf
        for T in (1, 2, 9, 40):
            t = np.array([0.5 * (lo + hi)]) if T == 1 else np.linspace(lo, hi, T)
            b, m = BT.counts(x, t), MK.counts(x, t)
            assert np.array_equal(b["components"] - b["holes"], m["euler"]), (n, kind, seed, T)
            assert np.array_equal(b["faces"], m["faces"]) and b["nan"] == m["nan"]
            assert np.array_equal(BT.ranks(x, t), MK.ranks(x, t))
            assert all(b[k].dtype == np.int64 and b[k].shape == (T,) for k in ("components", "holes", "faces"))


def one(q):
    """(components, holes) of the set of the nonzero pixels of q at the threshold 0.5."""
    r = BT.counts(np.array(q, np.float32), [0.5])
    return int(r["components"][0]), int(r["holes"][0])


def test_the_restatement_by_hand():
    assert one([[1]]) == (1, 0) and one([[0]]) == (0, 0)
    # a diagonal pair is one component; its two empty corners touch the rim
    assert one([[1, 0], [0, 1]]) == (1, 0)
    assert one([[1, 0, 0], [0, 0, 0], [0, 0, 1]]) == (2, 0)
    # a ring of eight around an empty centre
    assert one([[1, 1, 1], [1, 0, 1], [1, 1, 1]]) == (1, 1)
    # the ring's corners missing: still one component (8-connected), and the centre is still enclosed (4-connected)
    assert one([[0, 1, 0], [1, 0, 1], [0, 1, 0]]) == (1, 1)
    # a ring cut open by the rim: its pocket pixel lies on the map's first row and reaches outside
    assert one([[1, 0, 1], [1, 1, 1], [0, 0, 0]]) == (1, 0)
    # a pocket closed by pixels that themselves lie on the rim: the empty pixel (1, 1) touches no rim
    assert one([[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]) == (1, 1)
    # a hole that holds a component that holds a hole
    big = np.zeros((9, 9), np.float32)
    big[1:8, 1:8] = 1
    big[2:7, 2:7] = 0
    big[3:6, 3:6] = 1
    big[4, 4] = 0
    assert one(big) == (2, 2)
    # NaN is in no set and part of the complement: an enclosed NaN is a hole at every threshold
    x = np.ones((3, 3), np.float32)
    x[1, 1] = np.nan
    r = BT.counts(x, [-1.0, 0.5, 1.0, 2.0])
    assert list(r["components"]) == [1, 1, 1, 0] and list(r["holes"]) == [1, 1, 1, 0] and r["nan"] == 1
    assert list(r["faces"]) == [8, 8, 8, 0]
    # a checkerboard: one component; the interior empty squares are holes, the rim ones are not
    n = 7
    board = (np.add.outer(np.arange(n), np.arange(n)) % 2 == 0).astype(np.float32)
    empty_inside = int((board[1:-1, 1:-1] == 0).sum())
    assert one(board) == (1, empty_inside) and empty_inside == 12


@pytest.mark.parametrize("npix,thresholds,code,text", [
    (0, [0.0, 1.0], ERR_ARG, "npix must be positive"),
    (-4, [0.0], ERR_ARG, "npix must be positive"),
    (32769, [0.0], ERR_UNSUPPORTED, "npix = 32769 above 32768"),
    (16, [], ERR_ARG, "fewer than 1 threshold"),
    (16, list(range(1026)), ERR_ARG, "1026 thresholds, at most 1025"),
    (16, [np.nan], ERR_ARG, "thresholds must be finite"),
    (16, [0.0, 1.0, np.inf], ERR_ARG, "thresholds must be finite"),
    (16, [0.0, 1.0, 1.0], ERR_ARG, "thresholds must be strictly ascending"),
    (16, [2.0, 1.0, 0.0], ERR_ARG, "thresholds must be strictly ascending"),
    (16, [0.0], ERR_ARG, "null argument"),  # the numbers are good: only the handle is missing
    (32768, list(range(1025)), ERR_ARG, "null argument"),
])
def test_create_refusals_need_no_device(npix, thresholds, code, text):
    t = np.array(thresholds, np.float64)
    out = C.c_void_p(1)
    assert L.slicer_betti_create(None, npix, t.size, t.ctypes.data, C.byref(out)) == code
    assert _err() == "slicer_betti_create: " + text
    assert not out.value
    assert L.slicer_betti_create(None, npix, t.size, t.ctypes.data, None) == code  # a NULL `out`


def test_create_refuses_null_thresholds():
    out = C.c_void_p(1)
    assert L.slicer_betti_create(None, 16, 3, None, C.byref(out)) == ERR_ARG
    assert _err() == "slicer_betti_create: null argument"
    assert not out.value


def test_calls_without_a_handle():
    buf = np.zeros(8, np.int64)
    assert L.slicer_betti_run(None, buf.ctypes.data) == ERR_ARG
    assert _err() == "slicer_betti_run: null argument"
    assert L.slicer_betti_run_npix(None, buf.ctypes.data, 1) == ERR_ARG
    assert _err() == "slicer_betti_run_npix: null argument"
    assert L.slicer_betti_read(None, buf.ctypes.data, None, None, None) == ERR_ARG
    assert _err() == "slicer_betti_read: null handle"
    assert L.slicer_betti_destroy(None) == ERR_ARG
    assert slicer_amd.BETTI_MAX_THRESHOLDS == 1025 and slicer_amd.BETTI_MAX_NPIX == 32768
