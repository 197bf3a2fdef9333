"""The F32 bound of the tile deposit (tests/test_gpu_tile_deposit.py) kept honest without a GPU: a numpy
emulation of one heavy pixel's journey -- k contributions dealt to J work items, each item's LDS cell flushed with one
rounding, J f32 additions to the global cell -- stays inside (2J - 1) 2^-24 E with exact (integer) cells and inside that
plus k 2^-53 E with f64 cells, and leaves it with f32 cells, which the design rules out."""
import numpy as np
import pytest

import tile_np as tnp


def heavy_pixel(k, seed, le=-6):
    """k contributions of a constant mass just below 2^le, all exact multiples of the integer cells' quantum: a
    duplicated block of particles in a halo core -- a few distinct positions near the pixel centre, each many times, so
    that a sequential f32 sum rounds the same way again and again."""
    rng = np.random.default_rng(seed)
    m = np.float32(np.ldexp(0.998, le))
    c = (m * rng.choice(rng.uniform(0.5476, 0.5625, 3).astype(np.float32), k)).astype(np.float32)
    assert not tnp.not_quantum(c, le).any()
    return c


def exact_units(c, le):
    P = tnp.Pixels(np.zeros((len(c), 1), np.int64), c[:, None], 1, le)
    return int(P.exact()[0]), P


@pytest.mark.parametrize("k,J", [(16384, 1), (40000, 3), (65536, 4), (120000, 8)])
def test_bound_admits_exact_and_f64_cells_and_refuses_f32_cells(k, J):
    le = -6
    c = heavy_pixel(k, k + J, le)
    assert k > 1000 * J  # k >> J: the bound must not have room for a sum rounded k times
    part_of = (np.arange(k) * J) // k
    E, P = exact_units(c, le)
    ratio = {}
    for cells in ("int", "f64", "f32"):
        got = int(P.units(np.array([tnp.emulate_pixel(c, part_of, cells, le)], np.float32))[0])
        extra = k if cells == "f64" else 0
        ratio[cells] = abs(got - E) * (1 << 53) / (((2 * J - 1) * (1 << 29) + extra) * E)
    print(f"k {k}, J {J}: error / bound  integer cells {ratio['int']:.3g}, f64 cells {ratio['f64']:.3g}, "
          f"f32 cells {ratio['f32']:.3g}")
    assert ratio["int"] <= 1.0 and ratio["f64"] <= 1.0, ratio
    assert ratio["f32"] > 1.0, ratio


def test_whole_bin_cap_of_integer_cells():
    """65536 records of weight 0.5625 m on one cell wrap a u64 cell; kWholeRecsInt records never do."""
    le = -6
    unit = int(np.float64(np.float32(np.ldexp(0.998, le)) * np.float32(0.5625)) * 2.0 ** (49 - le))
    assert tnp.WHOLE_RECS * unit >= 1 << 64
    assert tnp.WHOLE_RECS_INT * ((9 << 49) // 16) < 1 << 64 and tnp.ITEM_RECS * ((9 << 49) // 16) < 1 << 64
    assert [int(tnp.parts_of(n, True)) for n in (0, 1, 32768, 32769, 65537)] == [0, 1, 1, 3, 5]
    assert [int(tnp.parts_of(n, False)) for n in (32769, 65536, 65537, 114688, 114689)] == [1, 1, 5, 7, 8]


def test_rn32_of_exact_integers():
    rng = np.random.default_rng(1)
    for v in rng.uniform(0.5, 1, 2000) * 2.0 ** rng.integers(-140, 60, 2000):
        n = int(np.ldexp(v, 200))  # 53 significant bits: float32(float64) is the single rounding
        assert tnp._rn32(n, -200) == np.float32(np.ldexp(float(n), -200))
    assert tnp._rn32((1 << 24) + 1, 0) == np.float32(1 << 24) and tnp._rn32((1 << 24) + 3, 0) == np.float32((1 << 24) + 4)
