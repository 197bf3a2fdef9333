"""The Minkowski-functional contract without a device: the restatement tests/minkowski_np.py
against a plain loop over faces, edges, vertices and thresholds, its Euler characteristic against a flood fill
(8-connected components of the set minus the holes of the 4-connected complement), its boundary against the count of
differing adjacent pairs, closed-form identities, answers by hand, the expectations of white noise,
minkowski_functionals against its stated expressions, and the refusals of slicer_minkowski_* that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import minkowski_np as MK
import slicer_amd
from slicer_amd import lensing

L = lensing._L
ERR_ARG, ERR_UNSUPPORTED = 2, 6
COUNTS = ("faces", "edges", "vertices", "boundary", "border")


def _err():
    return (L.slicer_last_error(None) or b"").decode()


def loop_counts(x, thresholds):
    """The contract, one element and one threshold at a time."""
    n, T = x.shape[0], len(thresholds)

    def inside(i, j, t):  # is face (i, j) in the set x >= t?  Outside the map and NaN: never
        return 0 <= i < n and 0 <= j < n and bool(float(x[i, j]) >= t)

    out = {k: [0] * T for k in COUNTS}
    for q, t in enumerate(thresholds):
        for i in range(n):
            for j in range(n):
                out["faces"][q] += inside(i, j, t)
        for i in range(n + 1):  # vertex (i, j): the corner shared by faces (i-1, j-1), (i-1, j), (i, j-1), (i, j)
            for j in range(n + 1):
                out["vertices"][q] += any(inside(a, b, t) for a in (i - 1, i) for b in (j - 1, j))
        for i in range(n + 1):  # horizontal edge between faces (i-1, j) and (i, j)
            for j in range(n):
                a, b = inside(i - 1, j, t), inside(i, j, t)
                out["edges"][q] += a or b
                if i in (0, n):
                    out["border"][q] += a or b
                else:
                    out["boundary"][q] += a != b
        for i in range(n):  # vertical edge between faces (i, j-1) and (i, j)
            for j in range(n + 1):
                a, b = inside(i, j - 1, t), inside(i, j, t)
                out["edges"][q] += a or b
                if j in (0, n):
                    out["border"][q] += a or b
                else:
                    out["boundary"][q] += a != b
    out["euler"] = [v - e + f for v, e, f in zip(out["vertices"], out["edges"], out["faces"])]
    out["nan"] = int(np.isnan(x).sum())
    return out


def components(mask, neighbours):
    """The number of connected components of the True cells of `mask`, by flood fill."""
    mask = mask.copy()
    count = 0
    for start in zip(*np.nonzero(mask)):
        if not mask[start]:
            continue
        count += 1
        mask[start] = False
        stack = [start]
        while stack:
            i, j = stack.pop()
            for di, dj in neighbours:
                a, b = i + di, j + dj
                if 0 <= a < mask.shape[0] and 0 <= b < mask.shape[1] and mask[a, b]:
                    mask[a, b] = False
                    stack.append((a, b))
    return count


N4 = [(-1, 0), (1, 0), (0, -1), (0, 1)]
N8 = N4 + [(-1, -1), (-1, 1), (1, -1), (1, 1)]


def euler_by_flood_fill(member):
    """8-connected components of the set minus its holes: the 4-connected components of the complement, padded by one
    ring so that everything that reaches outside the map is one component, minus that one."""
    return components(member, N8) - (components(~np.pad(member, 1), N4) - 1)


def maps_of(n, seed):
    rng = np.random.default_rng(seed + n)
    ties = rng.integers(-3, 4, (n, n)).astype(np.float32)
    smooth = rng.standard_normal((n, n)).astype(np.float32)
    holes = smooth.copy()
    holes.ravel()[::5] = np.nan
    holes.ravel()[1::7] = np.inf
    holes.ravel()[2::11] = -np.inf
    return ties, smooth, holes


THRESHOLDS = (np.array([0.0]), np.linspace(-2.0, 2.0, 9), np.array([-2.5, -1.0, 0.0, 0.125, 3.0]))


@pytest.mark.parametrize("n", range(1, 10))
def test_restatement_against_a_plain_loop(n):
    for x in maps_of(n, 100):
        for t in THRESHOLDS:  # (linspace(-2, 2, 9) holds the integer maps' own values)
            got = MK.counts(x, t)
            assert MK.same(got, loop_counts(x, [float(v) for v in t])), (n, t)
            assert got["faces"].dtype == np.int64 and got["euler"].dtype == np.int64


@pytest.mark.parametrize("n", list(range(1, 10)) + [17])
def test_euler_characteristic_is_components_minus_holes(n):
    t = np.linspace(-2.0, 2.0, 9)
    for x in maps_of(n, 200):
        got = MK.counts(x, t)
        for j, tj in enumerate(t):
            member = x.astype(np.float64) >= tj  # (NaN: False)
            assert got["euler"][j] == euler_by_flood_fill(member), (n, j)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 17, 40])
def test_boundary_is_the_number_of_differing_adjacent_pairs_and_border_the_sum_along_the_sides(n):
    t = np.linspace(-2.0, 2.0, 9)
    for x in maps_of(n, 300):
        got = MK.counts(x, t)
        for j, tj in enumerate(t):
            m = x.astype(np.float64) >= tj
            assert got["boundary"][j] == (m[1:] != m[:-1]).sum() + (m[:, 1:] != m[:, :-1]).sum()
            assert got["border"][j] == m[0].sum() + m[-1].sum() + m[:, 0].sum() + m[:, -1].sum()


@pytest.mark.parametrize("n", [1, 2, 7, 64, 129])
def test_closed_forms_of_the_full_and_the_empty_set(n):
    x = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
    t = np.concatenate([[-100.0], np.linspace(-3.0, 3.0, 31), [100.0]])
    got = MK.counts(x, t)
    full = {"faces": n * n, "edges": 2 * n * (n + 1), "vertices": (n + 1) ** 2, "boundary": 0, "border": 4 * n, "euler": 1}
    for k, v in full.items():
        assert got[k][0] == v, k
        assert got[k][-1] == 0, k
    for k in ("faces", "edges", "vertices", "border"):  # the sets are nested: these four never grow with the threshold
        assert np.all(np.diff(got[k]) <= 0), k
    assert got["nan"] == 0


def planted(n, at):
    x = np.zeros((n, n), np.float32)
    for a in at:
        x[a] = 1.0
    return MK.counts(x, [0.5])


def six(r):
    return [int(r[k][0]) for k in ("faces", "edges", "vertices", "boundary", "border", "euler")]


def test_answers_by_hand():
    assert six(planted(5, [(2, 2)])) == [1, 4, 4, 4, 0, 1]  # one pixel in the interior
    assert six(planted(5, [(0, 0)])) == [1, 4, 4, 2, 2, 1]  # one in a corner
    assert six(planted(5, [(0, 2)])) == [1, 4, 4, 3, 1, 1]  # one on a side
    two = planted(5, [(1, 1), (2, 2)])  # two diagonal neighbours share a vertex: one component (closed pixels)
    assert [int(two[k][0]) for k in ("faces", "edges", "vertices", "euler")] == [2, 8, 7, 1]
    ring = planted(5, [(i, j) for i in (1, 2, 3) for j in (1, 2, 3) if (i, j) != (2, 2)])
    assert six(ring) == [8, 24, 16, 16, 0, 0]  # one component, one hole
    n = 6  # a checkerboard: the black squares hang together by their corners, every white one inside the rim is a hole
    board = planted(n, [(i, j) for i in range(n) for j in range(n) if (i + j) % 2 == 0])
    whites_inside = sum(1 for i in range(1, n - 1) for j in range(1, n - 1) if (i + j) % 2 == 1)
    # every interior edge and vertex touches a black square; of the rim's edges the 2 n under a black one, and two corners not
    assert six(board) == [n * n // 2, 2 * n * (n - 1) + 2 * n, (n + 1) ** 2 - 2, 2 * n * (n - 1), 2 * n, 1 - whites_inside]
    assert six(planted(1, [(0, 0)])) == [1, 4, 4, 0, 4, 1]  # a map that is all border


@pytest.mark.parametrize("n", [64, 257, 1000])
def test_white_noise_has_its_expected_counts(n):
    x = np.random.default_rng(7919 * n).standard_normal((n, n)).astype(np.float32)
    t = np.array([-1.0, 0.0, 1.0])
    got = MK.counts(x, t)
    for j, tj in enumerate(t):
        p = 0.5 * math.erfc(tj / math.sqrt(2.0))
        q = 1.0 - p
        # (expectation, the number N of elements counted, the number m of indicators that share a pixel with one)
        want = {"faces": (n * n * p, n * n, 1),
                "boundary": (2 * n * (n - 1) * 2 * p * q, 2 * n * (n - 1), 7),
                "vertices": ((n - 1) ** 2 * (1 - q ** 4) + 4 * (n - 1) * (1 - q ** 2) + 4 * p, (n + 1) ** 2, 9),
                "edges": (2 * n * (n - 1) * (1 - q ** 2) + 4 * n * p, 2 * n * (n + 1), 7)}
        for k, (mean, N, m) in want.items():
            sigma = math.sqrt(N * m / 4.0)  # var of a sum of N indicators, each correlated with at most m (itself included)
            print(f"n {n} t {tj} {k}: (count - expectation) / sigma bound = {(got[k][j] - mean) / sigma:.3f}")
            assert abs(got[k][j] - mean) <= 5 * sigma, (n, tj, k)


def test_functionals_are_the_stated_expressions():
    n, angle = 37, 2.5
    x = np.random.default_rng(5).standard_normal((n, n)).astype(np.float32)
    read = MK.counts(x, np.linspace(-2, 2, 9))
    read["npix"] = n
    got = slicer_amd.minkowski_functionals(read, angle)
    theta = angle * math.pi / 180.0
    d = theta / n
    for j in range(9):
        assert got["v0"][j] == float(read["faces"][j]) / (float(n) * float(n))
        assert got["v1"][j] == float(read["boundary"][j]) * d / (4.0 * theta * theta)
        assert got["v1_with_border"][j] == (float(read["boundary"][j]) + float(read["border"][j])) * d / (4.0 * theta * theta)
        assert got["v2"][j] == float(read["euler"][j]) / (theta * theta)
    assert np.array_equal(got["thresholds"], read["thresholds"])
    assert all(got[k].dtype == np.float64 for k in ("v0", "v1", "v1_with_border", "v2"))
    assert slicer_amd.MINKOWSKI_MAX_THRESHOLDS == 1025


@pytest.mark.parametrize("npix,thresholds,code,text", [
    (0, [0.0, 1.0], ERR_ARG, "npix must be positive"),
    (-4, [0.0], ERR_ARG, "npix must be positive"),
    (131073, [0.0], ERR_UNSUPPORTED, "npix = 131073 above 131072"),
    (16, [], ERR_ARG, "fewer than 1 threshold"),
    (16, list(range(1026)), ERR_ARG, "1026 thresholds, at most 1025"),
    (16, [np.nan], ERR_ARG, "thresholds must be finite"),
    (16, [0.0, 1.0, np.inf], ERR_ARG, "thresholds must be finite"),
    (16, [-np.inf, 0.0, 1.0], ERR_ARG, "thresholds must be finite"),
    (16, [0.0, 1.0, 1.0], ERR_ARG, "thresholds must be strictly ascending"),
    (16, [0.0, 2.0, 1.0], ERR_ARG, "thresholds must be strictly ascending"),
    (16, [0.0], ERR_ARG, "null argument"),  # the numbers are good: only the handle is missing
    (131072, list(range(1025)), ERR_ARG, "null argument"),
])
def test_create_refusals_need_no_device(npix, thresholds, code, text):
    t = np.array(thresholds, np.float64)
    out = C.c_void_p(1)
    assert L.slicer_minkowski_create(None, npix, t.size, t.ctypes.data, C.byref(out)) == code
    assert _err() == "slicer_minkowski_create: " + text
    assert not out.value
    assert L.slicer_minkowski_create(None, npix, t.size, t.ctypes.data, None) == code


def test_create_refuses_null_thresholds():
    out = C.c_void_p(1)
    assert L.slicer_minkowski_create(None, 16, 3, None, C.byref(out)) == ERR_ARG
    assert _err() == "slicer_minkowski_create: null argument"
    assert not out.value


def test_calls_without_a_handle():
    buf = np.zeros(8, np.int64)
    assert L.slicer_minkowski_run(None, buf.ctypes.data) == ERR_ARG
    assert _err() == "slicer_minkowski_run: null argument"
    assert L.slicer_minkowski_run_npix(None, buf.ctypes.data, 1) == ERR_ARG
    assert _err() == "slicer_minkowski_run_npix: null argument"
    assert L.slicer_minkowski_read(None, buf.ctypes.data, None, None, None, None, None) == ERR_ARG
    assert _err() == "slicer_minkowski_read: null handle"
    assert L.slicer_minkowski_destroy(None) == ERR_ARG
