"""Host-side checks of the real-space two-point functions: the three forms of the restatement in
tests/xi_np.py against one another, slicer_xi_bins against enumeration, and the refusals of the edges.  No GPU.

The reference figure of the tolerance, the numpy FFT route against the direct pair sum in units of U_b (xi_np.unit),
is re-measured here and printed; xi_cases.REF_U holds the issue's 0.36."""
import math

import numpy as np
import pytest

import slicer_amd
import xi_cases
import xi_np

HOST_CASES = [c for c in xi_cases.CASES if c[0] <= 40] + [(97, 23, 120, 0)]


def test_brute_force_rotation_equals_c4_s4():
    n, L = 8, 7
    edges = [0.0, 1.0, 1.5, 2.0, 3.2, 5.0, 7.0]
    a1, a2, b1, b2 = (np.asarray(m[:n, :n]) for m in xi_cases.maps_for(12))
    for w in (None, np.asarray(xi_cases.weights_for(12, "smooth")[:n, :n])):
        fa1, fa2, fb1, fb2 = (xi_np.weighted(m, w) for m in (a1, a2, b1, b2))
        for fields in ((fa1, fa2, fa1, fa2), (fa1, fa2, fb1, fb2)):
            p1, p2, q1, q2 = fields
            win = lambda x, y: xi_np.window(x, y, L)
            plus, minus = xi_np.spin2_sums(win(p1, q1), win(p2, q2), win(p1, q2), win(p2, q1), n, edges)
            raw = (a1, a2, a1, a2) if q1 is fa1 else (a1, a2, b1, b2)
            bplus, bminus = xi_np.brute_spin2(*raw, w, edges)
            scale = float(np.sum(p1 * p1 + p2 * p2)) * 1e-13
            assert float(np.abs(plus - bplus).max()) <= scale
            assert float(np.abs(minus - bminus).max()) <= scale
            assert float(np.abs(minus).max()) > 1e3 * scale  # the comparison is of something


def test_point_mass_has_positive_tangential_shear():
    """gamma of row N6 around a point mass, -e^(2 i phi) / r^2 up to a positive factor (axis 0 is component 1), is
    tangential under the contract's sign: gamma_t = Re(-gamma e^(-2 i phi)) > 0."""
    d = np.arange(-6, 7, dtype=np.float64)
    dx, dy = np.meshgrid(d, d, indexing="ij")
    r2 = dx * dx + dy * dy
    r2[6, 6] = 1.0
    phi = np.arctan2(dy, dx)
    gamma = -np.exp(2j * phi) / r2
    gt = (-gamma * np.exp(-2j * phi)).real
    gt[6, 6] = 1.0
    assert np.all(gt > 0)


@pytest.mark.parametrize("n,L,P,bins", HOST_CASES)
def test_fft_route_matches_direct_sum(n, L, P, bins):
    worst = 0.0
    for kind in xi_cases.WEIGHTS:
        d = xi_cases.direct(n, L, bins, kind)
        assert d.P == P
        live = d.live()
        for i, j in ((0, 0), (0, 1), (2, 3)):
            ref, u = d.spin0(i, j)
            got = xi_np.bin_sum(xi_np.window_fft(d.f[i], d.f[j], L, P), n, d.edges)[live] / d.Wb[live]
            worst = max(worst, float((np.abs(got - ref[live]) / u[live]).max()))
        if d.w is not None:
            w64 = d.w.astype(np.float64)
            got = xi_np.bin_sum(xi_np.window_fft(w64, w64, L, P), n, d.edges)
            u = xi_np.unit(P, d.M, d.sumw2)
            has = d.M > 0
            worst = max(worst, float((np.abs(got - d.Wb)[has] / u[has]).max()))
    print(f"n={n} L={L} P={P}: numpy FFT route against the direct sum, at most {worst:.3g} U")
    assert worst <= xi_cases.REF_U


@pytest.mark.parametrize("n,L,P,bins", xi_cases.CASES)
def test_bins_equal_enumeration(n, L, P, bins):
    edges = xi_cases.edges_for(n, L, bins)
    got = slicer_amd.xi_bins(n, edges)
    N, M = xi_np.enumerate_bins(n, edges)
    assert got["padded"] == P == xi_np.padded_size(n, xi_np.max_lag(n, edges))
    assert np.array_equal(got["counts"], N) and np.array_equal(got["lags"], M)
    assert got["counts"].dtype == np.int64
    assert (M == 0).any()  # a bin with no lag


@pytest.mark.parametrize("n", [12, 15, 30, 33, 97])
def test_bins_edge_rules(n):
    top = math.sqrt(2.0) * (n - 1)
    for edges in ([3.0, 4.0, 5.0],                    # exact integer radii: m2 = 9, 16, 25 sit on edges
                  [0.0, 5.0],                          # 3-4-5: m2 = 25 only in the closed last bin
                  [0.0, 5.0, 6.0],                     # ... and in the next bin when 5 is an inner edge
                  [1.1, 1.3, top],                     # a bin with no lag; the farthest lag in the closed last bin
                  [0.5, 1.0],                          # m2 = 1 through the closed edge alone
                  [float(n - 2), float(n - 1)]):       # L = n - 1
        got = slicer_amd.xi_bins(n, edges)
        N, M = xi_np.enumerate_bins(n, edges)
        assert np.array_equal(got["counts"], N) and np.array_equal(got["lags"], M), edges
        L = xi_np.max_lag(n, edges)
        assert got["padded"] == xi_np.padded_size(n, L), edges
    assert slicer_amd.xi_bins(n, [0.0, 5.0])["lags"][0] == slicer_amd.xi_bins(n, [0.0, 5.0, 6.0])["lags"][0] + 12
    assert slicer_amd.xi_bins(n, [1.1, 1.3, top])["lags"].tolist() == [0, (2 * n - 1) ** 2 - 1 - 4]
    total = sum((n - abs(dx)) * (n - abs(dy)) for dx in range(1 - n, n) for dy in range(1 - n, n)) - n * n
    assert slicer_amd.xi_bins(n, [0.0, top])["counts"][0] == total


def test_padded_sizes():
    for n, last, P in ((4000, 96.0, 4096), (4096, 1024.0, 5120), (100, 27.5, 128), (8192, 8191.0, 16384)):
        assert slicer_amd.xi_bins(n, [0.0, last])["padded"] == P


REFUSALS = [
    (12, [0.0], 2, "slicer_xi_bins: fewer than 2 edges"),
    (12, [0.0, float("nan")], 2, "slicer_xi_bins: edges must be finite and non-negative"),
    (12, [0.0, float("inf")], 2, "slicer_xi_bins: edges must be finite and non-negative"),
    (12, [-1.0, 2.0], 2, "slicer_xi_bins: edges must be finite and non-negative"),
    (12, [0.0, 2.0, 2.0], 2, "slicer_xi_bins: edges must be strictly ascending"),
    (12, [0.0, 3.0, 2.0], 2, "slicer_xi_bins: edges must be strictly ascending"),
    (12, [0.0, 15.6], 2, "slicer_xi_bins: the last edge is beyond sqrt(2) (npix - 1)"),
    (1, [0.0, 1.0], 2, "slicer_xi_bins: npix = 1 outside 2..16383"),
    (16384, [0.0, 1.0], 2, "slicer_xi_bins: npix = 16384 outside 2..16383"),
    (2000, np.linspace(0.0, 600.0, 514), 6, "slicer_xi_bins: 513 bins, at most 512"),
    (9000, [0.0, 8999.0], 6, "slicer_xi_bins: no transform size up to 16384 holds npix + L = 9000 + 8999"),
]


@pytest.mark.parametrize("n,edges,code,text", REFUSALS)
def test_edge_refusals(n, edges, code, text):
    with pytest.raises(slicer_amd.SlicerError) as e:
        slicer_amd.xi_bins(n, edges)
    assert e.value.code == code
    assert text in str(e.value)


def test_null_edges_are_refused():
    lib = slicer_amd._lib.load()
    assert lib.slicer_xi_bins(12, 3, None, None, None, None) == 2
    assert lib.slicer_last_error(None) == b"slicer_xi_bins: the edges are required"
    assert slicer_amd.xi_bins(2000, np.linspace(0.0, 600.0, 513))["counts"].size == slicer_amd.XI_MAX_BINS
