"""The binned bispectrum contract on the host: the numpy restatement (tests/bispectrum_np.py)
against the plain double loop over the full plane, the exact triangle counts of slicer_bispectrum_triangles against the
restatement, their refusals, an analytic map of three plane waves, and the triple lists.  No GPU."""
import numpy as np
import pytest

import bispectrum_np
import slicer_amd

# Edge sets that reach past npix / 2 (the Nyquist row and column are in a bin); (1) has an empty bin (no integer m2 in
# [1.1^2, 1.3^2)), (2) an open triple: bins 0 and 2 are single shells whose sums never land in the other.
def edge_sets(n):
    return [
        np.array([0.0, 1.5, 0.4 * n, 0.75 * n]),
        np.array([0.0, 1.1, 1.3, 2.5, 0.3 * n, 0.8 * n]),
        np.array([0.9, 1.1, 0.45 * n, 0.55 * n, n]),
    ]


def test_edge_sets_have_an_empty_bin_and_an_open_triple():
    for n in (8, 12, 15, 16):
        assert bispectrum_np.full_plane_counts(n, edge_sets(n)[1])[1] == 0
        e = edge_sets(n)[2]
        tr = bispectrum_np.all_triples(len(e) - 1)
        T = np.rint(bispectrum_np.triangles(n, e, tr)).astype(np.int64)
        N = bispectrum_np.full_plane_counts(n, e)
        open_ = [(i, j, k) for (i, j, k), t in zip(tr, T) if t == 0 and N[i] and N[j] and N[k]]
        assert open_, n  # non-empty bins without a closed triangle
        assert N[-1] > 0 and bispectrum_np.full_plane_bins(n, e)[n // 2, n // 2] >= 0  # the corner mode is binned


@pytest.mark.parametrize("n", [8, 12, 15, 16])
def test_restatement_matches_the_double_loop(n):
    rng = np.random.default_rng(n)
    kappa = (rng.standard_normal((n, n)) ** 2).astype(np.float32)  # skewed: B != 0
    for e in edge_sets(n):
        tr = bispectrum_np.all_triples(len(e) - 1)
        ref = bispectrum_np.bispectrum(kappa, 5.0, e, tr)
        S, T = bispectrum_np.brute_force(kappa, e, tr)
        assert np.array_equal(np.rint(ref["triangles"]).astype(np.int64), T)
        assert np.abs(ref["triangles"] - T).max() < 1e-6
        scale = np.abs(S).max()
        assert scale > 0
        assert np.abs(float(n) ** 4 * ref["sums"] - S).max() <= 1e-9 * scale
        assert np.array_equal(np.isnan(ref["b"]), T == 0)
        theta = np.radians(5.0)
        nz = T > 0
        np.testing.assert_allclose(ref["b"][nz], theta ** 4 / float(n) ** 6 * S[nz] / T[nz], rtol=1e-9,
                                   atol=1e-9 * theta ** 4 / float(n) ** 6 * scale)


@pytest.mark.parametrize("n", [16, 30, 45, 49, 64])
def test_triangles_match_the_restatement(n):
    for e in (np.concatenate([[0.0], np.geomspace(1.0, 0.75 * n, 8)]), np.linspace(2.0, 0.3 * n, 7), edge_sets(n)[2]):
        B = len(e) - 1
        for tr in (None, slicer_amd.bispectrum_triples(B, "equilateral")):
            got = slicer_amd.bispectrum_triangles(n, e, tr)
            rows = bispectrum_np.all_triples(B) if tr is None else tr
            T = bispectrum_np.triangles(n, e, rows)
            assert np.abs(T - np.rint(T)).max() < 1e-3
            assert got.dtype == np.int64 and np.array_equal(got, np.rint(T).astype(np.int64))


def test_triangles_of_a_list_with_repeats_and_any_order():
    n, e = 30, np.array([0.0, 2.0, 5.0, 9.0, 14.0])
    full = slicer_amd.bispectrum_triangles(n, e)
    rows = bispectrum_np.all_triples(4)
    pick = [7, 0, 19, 7, 3, 3, 12]
    assert np.array_equal(slicer_amd.bispectrum_triangles(n, e, rows[pick]), full[pick])


def test_triangles_work_limit():
    with pytest.raises(slicer_amd.SlicerError) as err:
        slicer_amd.bispectrum_triangles(256, [0.0, 200.0], [[0, 0, 0]])  # 65535^2 mode pairs
    assert err.value.code == 6 and "2^31" in str(err.value)  # SLICER_ERR_UNSUPPORTED
    # the limit is on the sum over the triples: one prefix 2000 times over is refused, once is not
    e = [0.0, 20.0]
    N = int(bispectrum_np.full_plane_counts(64, e)[0])
    assert N * N < 2 ** 31 < 2000 * N * N
    assert slicer_amd.bispectrum_triangles(64, e, [[0, 0, 0]]).shape == (1,)
    with pytest.raises(slicer_amd.SlicerError) as err:
        slicer_amd.bispectrum_triangles(64, e, [[0, 0, 0]] * 2000)
    assert err.value.code == 6


def test_triangles_refusals():
    def refused(*args):
        with pytest.raises(slicer_amd.SlicerError) as err:
            slicer_amd.bispectrum_triangles(*args)
        assert err.value.code == 2, args  # SLICER_ERR_ARG
        return str(err.value)
    for edges in ([0.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 2.0], [0.0, float("inf")], [0.0, float("nan")]):
        msg = refused(16, edges)
        with pytest.raises(slicer_amd.SlicerError) as err:  # the same words as slicer_power_bins
            slicer_amd.power_bins(16, edges)
        assert msg.rsplit(": ", 1)[1] == str(err.value).rsplit(": ", 1)[1]
    e = [0.0, 2.0, 4.0, 6.0]
    for t in ([1, 0, 2], [0, 2, 1], [-1, 0, 1], [0, 1, 3], [3, 3, 3]):
        assert "triple" in refused(16, e, [t])
    refused(0, e)
    refused(16385, e)


def test_three_plane_waves():
    """kappa = A cos(a x) + B cos(b x) + C cos(c x), a + b + c = 0, each vector alone in its bin: the one triple of their
    bins has n^4 S = A B C n^6 / 4 (the triangles (a, b, c) and (-a, -b, -c), khat(+-a) = A n^2 / 2, ...), every other
    triple 0."""
    n = 32
    A, Bc, Cc = 0.7, -1.3, 0.45
    a, b, c = (3, 1), (-1, 4), (-2, -5)
    edges = np.array([0.0, 2.5, 3.5, 4.5, 5.2, 5.6, 9.0])
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    wave = lambda v: np.cos(2.0 * np.pi * (v[0] * i0 + v[1] * i1) / n)
    kappa = A * wave(a) + Bc * wave(b) + Cc * wave(c)
    bins = bispectrum_np.full_plane_bins(n, edges)
    hit = [int(bins[v[0] % n, v[1] % n]) for v in (a, b, c)]
    assert hit == [1, 2, 4]
    tr = bispectrum_np.all_triples(6)
    ref = bispectrum_np.bispectrum(kappa, 3.0, edges, tr)
    want = A * Bc * Cc * float(n) ** 6 / 4.0
    got = float(n) ** 4 * ref["sums"]
    for (i, j, k), s in zip(tr, got):
        if (i, j, k) == (1, 2, 4):
            assert abs(s - want) <= 1e-9 * abs(want)
        else:
            assert abs(s) <= 1e-9 * abs(want), (i, j, k)
    # and the estimator: B = theta^4 / n^6 * (n^4 S) / T with T from the exact count
    T = slicer_amd.bispectrum_triangles(n, edges, [[1, 2, 4]])[0]
    t = list(map(tuple, tr)).index((1, 2, 4))
    assert T > 0 and abs(ref["b"][t] - np.radians(3.0) ** 4 / float(n) ** 6 * want / T) <= 1e-9 * abs(ref["b"][t])


def test_triple_lists():
    for B in (1, 2, 5, 32):
        t = slicer_amd.bispectrum_triples(B, "all")
        assert t.dtype == np.int32 and t.shape == (B * (B + 1) * (B + 2) // 6, 3)
        assert np.all(t[:, 0] <= t[:, 1]) and np.all(t[:, 1] <= t[:, 2]) and t.min() == 0 and t.max() == B - 1
        rows = [tuple(r) for r in t]
        assert rows == sorted(set(rows))  # lexicographic, no repeats
        assert np.array_equal(t, bispectrum_np.all_triples(B))
        q = slicer_amd.bispectrum_triples(B, "equilateral")
        assert q.dtype == np.int32 and np.array_equal(q, np.repeat(np.arange(B, dtype=np.int32), 3).reshape(B, 3))
    assert slicer_amd.bispectrum_triples(32).shape[0] == 5984
    with pytest.raises(ValueError):
        slicer_amd.bispectrum_triples(4, "isosceles")
