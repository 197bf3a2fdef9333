"""slicer_l1norm_* on the device: the counts are slicer_amd.Peaks' exactly, the sums stay within
count_b 2^-53 S_b of the exact sum S_b (math.fsum, tests/starlet_np.py), the contract of include/slicer_amd.h."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import slicer_amd
import starlet_np as W
from slicer_amd import lensing

pytestmark = pytest.mark.gpu

L = lensing._L
ERR_ARG, ERR_STATE = 2, 3
# A chunk is 512 pixels (kL1Chunk = 64 lanes x 8), and workgroup g of G takes chunks g, g + G, ...  257^2 and 1000^2 are
# no multiple of a chunk.  1000^2 is 1954 chunks: on 256 CUs B = 1, 7, 64 run 1954 workgroups of one chunk each, and
# only B = 1024 (1280 workgroups) gives 674 of them a second chunk.  A third chunk, and with it the second rotation of
# the prefetched one, is met at ROUNDS_N alone (test_every_workgroup_takes_several_chunks).
SIZES = [1, 2, 3, 63, 64, 65, 257, 1000]
BINS = [1, 7, 64, 1024]                   # 1024: two copies of the sums a wave, 64: thirty-two, 1 and 7: sixty-four
ROUNDS_N, ROUNDS_CUS = 1801, 256          # the map on which every workgroup takes three chunks or more, and the CUs it was sized for


def resident_groups(lds_bytes, tiles, num_cus):
    """resident_groups of slicer_amd/csrc/slicer_rank_counts.hpp: kPerCu = 8, kMinGroups = 64, 160 KiB of LDS a CU."""
    per_cu = max(1, min(8, 160 * 1024 // lds_bytes))
    return min(tiles, max(64, per_cu * num_cus))


def l1_grid(n, B, num_cus):
    """(chunks, workgroups) of k_l1norm for an n x n map: l1_copies_log2, l1_lds and slicer_l1norm_create of
    slicer_amd/csrc/slicer_starlet.hip."""
    cl = 0
    while cl < 6 and ((B + 2) * 8 << (cl + 1)) <= 32 * 1024:
        cl += 1
    lds = (B + 1) * 8 + ((B + 2) * 8 << cl) + (B + 3) * 4
    chunks = (n * n + 511) // 512
    return chunks, resident_groups(lds, chunks, num_cus)


def device_cus():
    """The CUs of device 0 as slicer_create reads them: hipDeviceGetAttribute of hipDeviceAttributeMultiprocessorCount
    (63 in ROCm 7's hip_runtime_api.h), looked up through the library's own handle and so in the HIP runtime it is
    linked to.  (torch.cuda cannot be asked in this process: the wheel loads its own copy of the runtime, which finds no
    device once the library's has opened it.)"""
    value = C.c_int(0)
    L.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    assert L.hipDeviceGetAttribute(C.byref(value), 63, 0) == 0 and 1 <= value.value <= 4096, value.value
    return value.value


def fewest_chunks(n, B, num_cus):
    """The chunks of the workgroup that takes the fewest (the last one)."""
    chunks, G = l1_grid(n, B, num_cus)
    return chunks // G


# What the comments above and the sizing of ROUNDS_N claim, on ROUNDS_CUS CUs (no device needed)
assert [l1_grid(1000, B, ROUNDS_CUS) for B in BINS] == [(1954, 1954)] * 3 + [(1954, 1280)]
assert [l1_grid(ROUNDS_N, B, ROUNDS_CUS) for B in BINS] == [(6336, 2048)] * 3 + [(6336, 1280)]  # 192 workgroups take four
assert ROUNDS_N * ROUNDS_N - 6335 * 512 == 81                                                   # the last chunk is ragged
assert all(fewest_chunks(ROUNDS_N, B, ROUNDS_CUS) >= 3 for B in BINS)
# ... and 1775 is the smallest odd n with more than 3 * 8 * 256 chunks, the last of them ragged
assert min(n for n in range(1, 2000, 2) if (n * n + 511) // 512 > 3 * 8 * ROUNDS_CUS and n * n % 512) == 1775
assert all(fewest_chunks(1775, B, ROUNDS_CUS) >= 3 for B in BINS) and fewest_chunks(1773, 7, ROUNDS_CUS) == 2


@pytest.fixture(scope="module")
def slicer():
    with slicer_amd.Slicer(0, max_chunk=1 << 16) as s:
        yield s


@functools.lru_cache(maxsize=4)
def make_map(n, seed=0):
    rng = np.random.default_rng(7901 * n + seed)
    x = (np.exp(rng.standard_normal((n, n), np.float32)) - np.float32(math.exp(0.5))).astype(np.float32)
    x.setflags(write=False)
    return x


def run(s, x, edges, twice=False):
    """(L1Norm.read(), Peaks.read()) of the map x; twice: the l1norm runs again and must give the same bytes."""
    n = x.shape[0]
    d = s.to_device(np.ascontiguousarray(x))
    try:
        with slicer_amd.L1Norm(s, n, edges) as l1, slicer_amd.Peaks(s, n, edges) as pk:
            l1.run(d)
            got = l1.read()
            if twice:
                l1.run(d)
                again = l1.read()
                assert again["l1"].tobytes() == got["l1"].tobytes() and again["counts"].tobytes() == got["counts"].tobytes()
                assert (again["below_l1"], again["above_l1"]) == (got["below_l1"], got["above_l1"])
            pk.run(d)
            return got, pk.read()
    finally:
        s.free(d)


def check(s, x, edges, twice=False):
    got, pk = run(s, x, edges, twice)
    ref = W.l1norm(x, edges)
    # the counts: Peaks' and the restatement's, exactly
    assert np.array_equal(got["counts"], pk["pdf"]) and np.array_equal(got["counts"], ref["counts"])
    assert (got["below"], got["above"], got["nan"]) == (int(pk["below"][0]), int(pk["above"][0]), pk["nan"])
    assert (got["below"], got["above"], got["nan"]) == (ref["below"], ref["above"], ref["nan"])
    assert got["counts"].sum() + got["below"] + got["above"] + got["nan"] == x.size
    # the sums: |sum_b - S_b| <= count_b 2^-53 S_b
    sums = np.concatenate([got["l1"], [got["below_l1"], got["above_l1"]]])
    exact = np.concatenate([ref["l1"], [ref["below_l1"], ref["above_l1"]]])
    counts = np.concatenate([ref["counts"], [ref["below"], ref["above"]]]).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(sums - exact) <= counts * 2.0 ** -53 * exact) | ((sums == exact) & np.isinf(exact))
    assert ok.all(), (x.shape[0], len(edges) - 1, np.argwhere(~ok)[:4].tolist())
    return got


@pytest.mark.parametrize("n", SIZES)
def test_counts_are_peaks_and_sums_stay_within_the_contract(slicer, n):
    x = make_map(n)
    for B in BINS:
        got = check(slicer, x, slicer_amd.peaks_edges(-1.2, 2.5, B), twice=B == 64)
        assert n < 63 or (got["below"] > 0 and got["above"] > 0 and got["counts"].min(initial=1) >= 0)


def test_all_pixels_in_one_bin(slicer):
    n = 130
    x = (np.float32(1.0) + np.abs(make_map(n)) * np.float32(1e-3)).astype(np.float32)  # all within [1, 1.1)
    for B in (1, 64):
        edges = slicer_amd.peaks_edges(1.0, 1.1 * B, B)  # the first bin is [1, 2.1)
        got = check(slicer, x, edges, twice=True)
        assert got["counts"][0] == n * n and got["counts"][1:].sum() == 0 and not got["l1"][1:].any()
    got = check(slicer, x, [2.0, 3.0])
    assert got["below"] == n * n and got["counts"][0] == 0 and got["l1"][0] == 0.0 and got["below_l1"] > n * n
    got = check(slicer, -x, [-0.5, 0.0, 0.5])
    assert got["below"] == n * n and got["below_l1"] > n * n  # |x| is summed, not x


def test_pixels_exactly_on_edges(slicer):
    edges = np.array([-2.0, -0.5, 0.0, 0.25, 1.0, 3.0])
    n = 64
    rng = np.random.default_rng(5)
    x = rng.choice(np.concatenate([edges, [-2.5, 3.5, 0.125]]).astype(np.float32), size=(n, n))
    got = check(slicer, x, edges)
    on = lambda v: int((x == np.float32(v)).sum())
    # an edge belongs to the bin it opens; the last edge closes the last bin
    assert got["counts"].tolist() == [on(-2.0), on(-0.5), on(0.0) + on(0.125), on(0.25), on(1.0) + on(3.0)]
    assert got["below"] == on(-2.5) and got["above"] == on(3.5)
    # eighths: every sum is exact
    assert got["l1"].tolist() == [2.0 * on(-2.0), 0.5 * on(-0.5), 0.125 * on(0.125), 0.25 * on(0.25), on(1.0) + 3.0 * on(3.0)]
    assert got["below_l1"] == 2.5 * on(-2.5) and got["above_l1"] == 3.5 * on(3.5)


def test_nan_and_infinite_pixels(slicer):
    n = 65
    x = make_map(n).copy()
    x[3, 7] = x[64, 64] = np.nan
    x[10, 0] = np.inf
    x[0, 10] = x[33, 33] = -np.inf
    got = check(slicer, x, slicer_amd.peaks_edges(-1.0, 2.0, 7))
    assert got["nan"] == 2 and got["below_l1"] == math.inf and got["above_l1"] == math.inf
    assert np.isfinite(got["l1"]).all()
    # without the infinities the outside sums are finite, and the NaNs enter no sum
    x[10, 0] = x[0, 10] = x[33, 33] = 0.0
    got = check(slicer, x, slicer_amd.peaks_edges(-1.0, 2.0, 7))
    assert got["nan"] == 2 and math.isfinite(got["below_l1"]) and math.isfinite(got["above_l1"])


@pytest.mark.parametrize("n", [100, 1000])
def test_an_integer_valued_map_sums_exactly(slicer, n):
    rng = np.random.default_rng(n)
    x = rng.integers(-40, 41, size=(n, n)).astype(np.float32)
    for B in (7, 64):
        edges = slicer_amd.peaks_edges(-32.0, 32.0, B)
        got, _ = run(slicer, x, edges, twice=True)
        ref = W.l1norm(x, edges)
        assert got["l1"].tolist() == ref["l1"].tolist() and np.array_equal(got["counts"], ref["counts"])
        assert (got["below_l1"], got["above_l1"]) == (ref["below_l1"], ref["above_l1"])


@pytest.mark.parametrize("part", ["lognormal", "integers", "non_finite"])
def test_every_workgroup_takes_several_chunks(slicer, part):
    """ROUNDS_N^2 pixels are 6336 chunks: on 256 CUs workgroups 0 ... 191 of 2048 (B = 1, 7, 64) take four chunks and the
    rest three, the 1280 of B = 1024 four or five, so the grid-stride loop, the prefetch of the next chunk and the
    rotation cur = nxt run more than twice in every workgroup; the last chunk holds 81 pixels.  The bounds are the
    header's: counts exact, |sum - S| <= count 2^-53 S against math.fsum."""
    n, cus = ROUNDS_N, device_cus()
    print(f"{cus} CUs: (chunks, workgroups) = {[l1_grid(n, B, cus) for B in BINS]}")
    for B in BINS:  # on another device the map has to be sized anew: fail, do not pass beside the point
        assert fewest_chunks(n, B, cus) >= 3, (cus, B, l1_grid(n, B, cus))
    if part == "lognormal":
        for B in BINS:
            got = check(slicer, make_map(n), slicer_amd.peaks_edges(-1.2, 2.5, B), twice=True)
            assert got["below"] > 0 and got["above"] > 0
    elif part == "integers":  # a dropped, repeated or misplaced chunk changes a sum or a count exactly
        x = np.random.default_rng(n).integers(-40, 41, size=(n, n)).astype(np.float32)
        for B in (7, 1024):
            edges = slicer_amd.peaks_edges(-32.0, 32.0, B)
            got, _ = run(slicer, x, edges, twice=True)
            ref = W.l1norm(x, edges)
            assert got["l1"].tolist() == ref["l1"].tolist() and np.array_equal(got["counts"], ref["counts"])
            assert (got["below_l1"], got["above_l1"]) == (ref["below_l1"], ref["above_l1"])
            assert (got["below"], got["above"], got["nan"]) == (ref["below"], ref["above"], 0)
    else:  # three NaNs, +inf and -inf in the last, ragged chunk and in a chunk of a workgroup's third round
        B = 7
        chunks, G = l1_grid(n, B, cus)
        flat = make_map(n).copy().ravel()
        for chunk in (chunks - 1, 2 * G + G // 3):
            assert 2 * G <= chunk < chunks
            at = chunk * 512 + np.array([0, 17, 64, 70, 80])  # lanes 0 and 17 of q = 0; lanes 0, 6 and 16 of q = 1 (the map's last pixel)
            assert at[-1] < n * n
            flat[at] = [np.nan, np.inf, np.nan, -np.inf, np.nan]
        got = check(slicer, flat.reshape(n, n), slicer_amd.peaks_edges(-1.2, 2.5, B), twice=True)
        assert got["nan"] == 6 and got["below_l1"] == math.inf and got["above_l1"] == math.inf
        assert got["counts"].sum() + got["below"] + got["above"] == n * n - 6 and np.isfinite(got["l1"]).all()


def test_run_npix_and_the_scales_of_a_starlet(slicer):
    n, m = 96, 41
    x = make_map(n)
    edges = slicer_amd.peaks_edges(-0.5, 0.5, 16)
    d = slicer.to_device(x)
    dm = slicer.to_device(make_map(m))
    try:
        with slicer_amd.Starlet(slicer, n, 3) as st, slicer_amd.L1Norm(slicer, n, edges) as l1:
            st.run(d)
            for scale in range(4):
                l1.run_scale(st, scale)
                got, ref = l1.read(), W.l1norm(st.read(scale), edges)
                assert np.array_equal(got["counts"], ref["counts"])
                assert (np.abs(got["l1"] - ref["l1"]) <= ref["counts"] * 2.0 ** -53 * ref["l1"]).all()
            l1.run(dm, m)  # a smaller map on the same handle is a handle of that size
            small = l1.read()
        fresh, _ = run(slicer, make_map(m), edges)
        assert small["l1"].tobytes() == fresh["l1"].tobytes() and np.array_equal(small["counts"], fresh["counts"])
    finally:
        slicer.free(d)
        slicer.free(dm)


def test_state_and_argument_refusals(slicer):
    n = 16
    d = slicer.to_device(np.zeros(n * n, np.float32))
    e = np.array([-1.0, 0.0, 1.0])
    lh = C.c_void_p()
    assert L.slicer_l1norm_create(slicer._h, n, 3, e.ctypes.data, C.byref(lh)) == 0
    err = lambda: (L.slicer_last_error(slicer._h) or b"").decode()
    try:
        counts, sums = np.ones(2, np.int64), np.ones(2, np.float64)
        assert L.slicer_l1norm_read(lh, counts.ctypes.data, None, None, None, None, None, None) == ERR_STATE
        assert err() == "slicer_l1norm_read before any slicer_l1norm_run"
        assert L.slicer_l1norm_run(lh, None) == ERR_ARG and err() == "slicer_l1norm_run: null argument"
        for bad in (0, 17):
            assert L.slicer_l1norm_run_npix(lh, d, bad) == ERR_ARG
            assert err() == f"slicer_l1norm_run_npix: npix = {bad} outside 1..16"
        assert L.slicer_l1norm_run(lh, d) == 0
        assert L.slicer_l1norm_read(lh, None, None, None, None, None, None, None) == 0
        assert L.slicer_l1norm_read(lh, counts.ctypes.data, sums.ctypes.data, None, None, None, None, None) == 0
        assert counts.tolist() == [0, n * n] and sums.tolist() == [0.0, 0.0]
    finally:
        L.slicer_l1norm_destroy(lh)
        slicer.free(d)
    with pytest.raises(slicer_amd.SlicerError):
        slicer_amd.L1Norm(slicer, n, [1.0, 1.0])


def test_the_kernels_show_in_the_profile(slicer):
    n = 64
    d = slicer.to_device(make_map(n))
    try:
        with slicer_amd.L1Norm(slicer, n, [0.0, 1.0]) as l1:
            slicer.profile_reset()
            slicer.profile_enable(True)
            l1.run(d)
            l1.run(d, 32)
            l1.read()
            prof = slicer.profile_get()
            slicer.profile_enable(False)
        assert prof["l1norm"][0] == 2 and prof["l1norm_finish"][0] == 2
    finally:
        slicer.free(d)
