"""tests/golden/k1_edges.npz without a GPU: every class label is recomputed from the raw positions with
np_restatement (k1_edges_np.classify), and the classes hold the counts the GPU tests rely on.  A stale or mislabelled
fixture fails here."""
import os

import numpy as np
import pytest

import golden_util  # noqa: F401  (tests/ on the path)
import k1_edges_np as ke
import oracle

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "k1_edges.npz")


@pytest.fixture(scope="module")
def data():
    return np.load(FIXTURE)


def count(lab, bit):
    return int(((lab & bit) != 0).sum())


@pytest.mark.parametrize("name,npix,pow2_bounds", [("a", 512, True), ("b", 300, False)])
def test_labels_are_current_and_classes_are_full(data, name, npix, pow2_bounds):
    g = ke.Geometry.from_params(data[name + "_params"])
    raw, stored = data[name + "_pos"], data[name + "_label"]
    assert raw.dtype == np.float32 and g.npix == npix and g.fov == 0.25
    assert all(float(np.float32(c)) == c and c >= 2.0 ** -20 for c in g.center)  # the fast kernel's condition
    assert all((float(np.float32(e)) == e) == pow2_bounds for e in g.edges)
    lab, e = ke.classify(raw, g)
    assert np.array_equal(lab, stored), "labels of the fixture are stale: rerun tests/golden/make_k1_edges.py"
    # T
    assert count(lab, ke.T) >= 300 and count(lab, ke.T_BELOW) >= 64 and count(lab, ke.T_ABOVE) >= 64
    t = (lab & ke.T) != 0
    td = np.minimum(np.abs(e.tdx), np.abs(e.tdy))
    assert td[t].max() <= ke.WINDOW and e.selected[t].all()
    close = (lab & (ke.T_BELOW | ke.T_ABOVE)) != 0
    assert td[close].max() <= ke.CLOSE
    # R
    assert count(lab, ke.R) >= 300
    # F, P: both sides, each axis
    for bit in (ke.F_DEC_IN, ke.F_DEC_OUT, ke.F_RA_IN, ke.F_RA_OUT):
        assert count(lab, bit) >= 8, bit
    assert count(lab, ke.P_DEC) >= 100 and count(lab, ke.P_RA) >= 100
    # Z: every threshold, on it and one step below
    edge = ke.z_edge(e.z, g)[(lab & ke.Z) != 0]
    assert [int((edge == k).sum()) >= 4 for k in range(10)] == [True] * 10, np.bincount(edge, minlength=10)
    pretest(lab, e, g)
    if npix == 300:
        assert count(lab, ke.C) >= 32
        c = (lab & ke.C) != 0
        dl = 1.0 / np.float64(npix)
        for v in (e.xs, e.ys):
            assert {0.25, 0.5, 0.75, 1.0} <= set(np.unique(v[c]).tolist())
            # the reference's division and the exact product part at 0.75 alone: cells 224 | 225, which share every
            # power-of-two tile and lie on the map -- the one place where the kernel's cell could differ leaves the
            # maps as they are; the entries still run the `tx == fx` branch into the exact epilogue
            part = c & (np.floor(v.astype(np.float64) / dl) != np.floor(v.astype(np.float64) * npix))
            assert set(np.unique(v[part]).tolist()) == {0.75} and int(part.sum()) >= 4


def pretest(lab, e, g):
    """The f32 pre-test lets every selected entry through -- also without the margin of k_ra (the argument is in
    k1_edges_np.pretest_outside): checked on the entries next to the limit, of which there are >= 150."""
    near = e.selected & ((lab & (ke.P | ke.FC)) != 0)
    assert near.sum() >= 150
    assert not (e.selected & ke.pretest_outside(e, g, margin=True)).any()
    assert not (e.selected & ke.pretest_outside(e, g, margin=False)).any() and count(lab, ke.M) == 0


def test_fixture_at_the_wide_field(data):
    """Fixture "c" (300^2, fov 0.5, the 15-term series): both sides of the FOV limit and the pre-test's margin only."""
    g = ke.Geometry.from_params(data["c_params"])
    lab, e = ke.classify(data["c_pos"], g)
    assert np.array_equal(lab, data["c_label"]) and g.fov == 0.5 and g.npix == 300
    for bit in (ke.F_DEC_IN, ke.F_DEC_OUT, ke.F_RA_IN, ke.F_RA_OUT):
        assert count(lab, bit) >= 8, bit
    assert count(lab, ke.P_DEC) >= 64 and count(lab, ke.P_RA) >= 64
    pretest(lab, e, g)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_the_oracle_sees_the_same_entries(data, name):
    """np_restatement and the oracle agree on the selected set, the plane and the f32 map coordinates of the fixture:
    what the labels say holds for the reference the GPU tests compare with."""
    g = ke.Geometry.from_params(data[name + "_params"])
    raw = data[name + "_pos"]
    _, e = ke.classify(raw, g)
    x, y, z = oracle.transform(raw, g.box, g.sgn, g.face, g.center, g.rcase)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((x, e.x), (y, e.y), (z, e.z)))
    for p in range(4):
        xs, ys, _, idx = oracle.select_project(x, y, z, None, 1.0, g.edges[p], g.edges[p + 1], g.box, 0, g.fov, g.npix,
                                               want_index=True)
        mine = np.nonzero(e.selected & (e.plane == p))[0]
        assert np.array_equal(idx, mine)
        assert np.array_equal(xs.view(np.uint32), e.xs[mine].view(np.uint32))
        assert np.array_equal(ys.view(np.uint32), e.ys[mine].view(np.uint32))
