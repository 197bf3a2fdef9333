"""The host side of the E/B pseudo-C_l, no GPU: slicer_amd.spin_phases bit for bit against the
restatement in tests/pcl_shear_np.py, and the restatement's two routes to the coupling matrices against each other."""
import ctypes as C

import numpy as np
import pytest

import pcl_np
import pcl_shear_np
import power_np
import slicer_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def chiral(n):
    """A diagonal slab with holes: no mirror symmetry, so that X_2 and X_4 do not vanish."""
    i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    w = (np.abs(i0 - i1) <= max(2, n // 4)).astype(np.float32)
    w[n // 3, n // 3 + 1] = 0.0
    w[n // 2:n // 2 + 2, n // 2 - 1] = 0.0
    w[(2 * n) // 3 + 1, (2 * n) // 3] = 0.0
    return w


def log_edges(n):
    return np.concatenate([[0.0], np.geomspace(1.0, n * 0.75, 8)])


def unit_edges(n):
    return np.arange(n // 2 + 1, dtype=np.float64)


@pytest.mark.parametrize("spin", [2, 4])
@pytest.mark.parametrize("n", [2, 12, 15, 16, 45, 128])
def test_spin_phases_are_the_restatement_bit_for_bit(n, spin):
    c, s = slicer_amd.spin_phases(n, spin)
    rc, rs = pcl_shear_np.phases(n, spin)
    assert c.shape == s.shape == (n, n // 2 + 1)
    assert np.array_equal(bits(c), bits(rc)) and np.array_equal(bits(s), bits(rs))
    assert c[0, 0] == 1.0 and s[0, 0] == 0.0
    if n % 2 == 0:
        assert not s[n // 2].any() and not s[:, n // 2].any()
    # off the Nyquist lines the rotation is one: c^2 + s^2 = 1 within a few roundings
    j0 = np.abs(np.fft.fftfreq(n, 1.0 / n).round())[:, None] + np.zeros((1, n // 2 + 1))
    j1 = np.arange(n // 2 + 1)[None, :] + np.zeros((n, 1))
    off = np.ones(c.shape, bool) if n % 2 else (j0 != n // 2) & (j1 != n // 2)
    assert np.all(np.abs(c * c + s * s - 1.0)[off] <= 8 * 2.0 ** -52)


def test_spin_phases_refusals():
    L = slicer_amd._lib.load()
    buf = np.zeros((4, 3))
    for n, spin in ((1, 2), (0, 4), (-3, 2), (4, 0), (4, 1), (4, 3), (4, 8)):
        assert L.slicer_pcl2_phases(n, spin, buf.ctypes.data, buf.ctypes.data) == 2  # SLICER_ERR_ARG
    assert L.slicer_pcl2_phases(4, 2, None, buf.ctypes.data) == 2
    assert L.slicer_pcl2_phases(4, 2, buf.ctypes.data, None) == 2
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.spin_phases(4, 3)
    assert C.c_int(L.slicer_pcl2_phases(4, 4, buf.ctypes.data, buf.ctypes.data)).value == 0


@pytest.mark.parametrize("n", [12, 15, 16])
def test_both_routes_agree_under_a_chiral_mask(n):
    w = chiral(n)
    for edges in (log_edges(n), unit_edges(n)):
        for spin in (2, 4):
            Mf, Xf = pcl_shear_np.coupling_fft(w, edges, spin)
            Mb, Xb = pcl_shear_np.coupling_brute(w, edges, spin)
            assert np.abs(Mf - Mb).max() <= 1e-14 and np.abs(Xf - Xb).max() <= 1e-14
            if spin == 4:
                assert np.abs(Xb).max() > 1e-4  # the X path is not tested on zeros


@pytest.mark.parametrize("n", [12, 15, 16])
def test_constant_masks(n):
    seen = False  # log_edges reach past n / 2: some bin holds Nyquist-line modes off the axes
    for edges in (log_edges(n), unit_edges(n)):
        counts, _ = power_np.binned_sums(n, edges)
        nz = counts > 0
        idx = power_np.bin_index(power_np.m2_rows(n, 0, n), edges)
        j0 = np.abs(np.fft.fftfreq(n, 1.0 / n).round())[:, None] + np.zeros((1, n // 2 + 1))
        j1 = np.arange(n // 2 + 1)[None, :] + np.zeros((n, 1))
        on_nyq = (n % 2 == 0) & ((j0 == n // 2) | (j1 == n // 2))
        for c in (1.0, 0.5):
            w = np.full((n, n), c, np.float32)
            for spin in (2, 4):
                Cs, Ss = pcl_shear_np.phases(n, spin)
                # the modes whose sine was averaged away (on the axes and, for spin 4, the diagonal it was 0 anyway)
                lost = 1.0 - (Cs * Cs + Ss * Ss) > 1e-6
                assert not (lost & ~on_nyq).any()
                touched = np.zeros(len(counts), bool)
                touched[np.unique(idx[lost & (idx >= 0)])] = True
                seen |= bool(touched.any())
                _, (d,) = power_np.binned_sums(n, edges, [Cs * Cs + Ss * Ss])
                diag = np.where(nz, d / np.maximum(counts, 1), 0.0)
                for route in (pcl_shear_np.coupling_fft, pcl_shear_np.coupling_brute):
                    M, X = route(w, edges, spin)
                    assert np.abs(X).max() <= 1e-14
                    assert np.abs(M - c * c * np.diag(diag)).max() <= 1e-14
                assert np.all(np.abs(diag[nz & ~touched] - 1.0) <= 1e-14)
                assert np.all(diag[nz & touched] < 1.0 - 1e-6 / counts[nz & touched])
    assert (n % 2 == 0) == seen


def test_block_systems_reduce_to_the_scalar_case():
    """Without chirality (X = 0) and with M_2 = M_4 = M_0 the systems decouple to M_0 on every spectrum, and a pure-E
    input stays pure E."""
    n = 12
    edges = unit_edges(n)
    M0 = pcl_np.coupling_fft(pcl_np.mask(n, 3.0), edges)
    Z = np.zeros_like(M0)
    B = M0.shape[0]
    s4 = pcl_shear_np.system4(M0, M0, Z)
    assert np.array_equal(s4[:B, :B], M0) and not s4[:B, B:].any()
    s2 = pcl_shear_np.system2(M0, Z)
    assert np.array_equal(s2[B:, B:], M0) and not s2[:B, B:].any()
    counts, _ = power_np.binned_sums(n, edges)
    ee = np.linspace(1.0, 2.0, B)
    x = pcl_shear_np.solve_blocks(s4, [M0 @ ee, np.zeros(B), np.zeros(B), np.zeros(B)], counts > 0)
    assert np.abs(x[0] - ee).max() <= 1e-12 and np.abs(x[1:]).max() <= 1e-12
