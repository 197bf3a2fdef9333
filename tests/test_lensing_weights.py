"""Host weights of the Born convergence maps (slicer_lensing_weights) against an independent
numpy / scipy restatement (tests/kappa_np.py).  No GPU needed."""
import json
import os

import numpy as np
import pytest

import kappa_np
import slicer_amd
from slicer_amd import SlicerError
from test_driver import make_cone, run


def cone_planes(tmp_path):
    ini, _, out = make_cone(tmp_path)
    plan_path = str(tmp_path / "plan.json")
    r = run([ini, "--plan-only", "--dump-plan", plan_path])
    assert r.returncode == 0, r.stderr
    planes = json.load(open(plan_path))["planes"]
    rows = [ln.split() for ln in open(os.path.join(out, "cone_planes_list_t0.txt")).read().strip().split("\n")]
    ld = np.array([p["ld"] for p in planes])
    ld2 = np.array([p["ld2"] for p in planes])
    zsnap = np.array([float(r[6]) for r in rows])
    return ld, ld2, zsnap


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300), initial=0.0))


@pytest.mark.parametrize("w0", [-1.0, -1.3])
def test_weights_match_the_restatement_on_the_cone(tmp_path, w0):
    ld, ld2, zsnap = cone_planes(tmp_path)
    assert len(ld) >= 20 and zsnap.max() > 0
    got = slicer_amd.plane_weights(0.3, 0.7, w0, 2.0, 32, ld, ld2, zsnap)
    c, zlo, zup, zl, chil = kappa_np.weights(0.3, w0, 2.0, 32, ld, ld2, zsnap)
    assert zlo[0] == 0 and got["zlo"][0] == 0
    assert rel(got["zlo"][1:], zlo[1:]) <= 1e-9
    for k, v in (("zup", zup), ("zl", zl), ("chil", chil)):
        assert rel(got[k], v) <= 1e-9, k
    assert np.array_equal(got["zs"], got["zup"])
    assert np.array_equal(got["c"] == 0, c == 0)
    assert rel(got["c"][c != 0], c[c != 0]) <= 1e-9
    # a source list of our own, between the plane edges
    zs = [0.05, float(zup[7]) + 5e-5, 0.19]
    got = slicer_amd.plane_weights(0.3, 0.7, w0, 2.0, 32, ld, ld2, zsnap, sources=zs)
    c, *_ = kappa_np.weights(0.3, w0, 2.0, 32, ld, ld2, zsnap, zs=zs)
    assert np.array_equal(got["c"] == 0, c == 0)
    assert rel(got["c"][c != 0], c[c != 0]) <= 1e-9


def test_source_rule_and_growth_switch():
    ld = np.arange(10) * 50.0
    ld2 = ld + 50.0
    zsnap = np.repeat([0.0, 0.1], 5)
    base = slicer_amd.plane_weights(0.3, 0.7, -1.0, 5.0, 64, ld, ld2, zsnap)
    zup = base["zup"]
    # a plane counts for a source when z(ld2) <= zs + 1e-4, and only then
    for s, z in enumerate(zup):
        assert np.all(base["c"][s][zup <= z + 1e-4] > 0) and np.all(base["c"][s][zup > z + 1e-4] == 0)
    just = slicer_amd.plane_weights(0.3, 0.7, -1.0, 5.0, 64, ld, ld2, zsnap, sources=[zup[3] - 0.99e-4, zup[3] - 1.01e-4])
    assert just["c"][0][3] > 0 and just["c"][1][3] == 0 and just["c"][1][2] > 0
    # growth off: g = 1, i.e. the ratio of the two is D+(zl) / D+(zsnap); for flat LCDM the closed form
    # D ~ H(a) int_0^a da' / (a' H(a'))^3 holds
    off = slicer_amd.plane_weights(0.3, 0.7, -1.0, 5.0, 64, ld, ld2, zsnap, growth=False)
    live = base["c"] > 0
    g = base["c"][live] / off["c"][live]
    cos = kappa_np.Flat(0.3)

    def closed(z):
        a = 1 / (1 + z)
        from scipy.integrate import quad
        h = lambda x: np.sqrt(0.3 * x ** -3 + 0.7)  # noqa: E731
        return h(a) * quad(lambda x: 1 / (x * h(x)) ** 3, 0, a, epsabs=0, epsrel=1e-13)[0]
    expect = np.array([[closed(base["zl"][p]) / closed(zsnap[p]) for p in range(10)]] * 10)[live]
    assert rel(g, expect) <= 1e-8
    # the restatement's ODE agrees with the closed form as well
    dz = cos.growth(base["zl"]) / cos.growth(zsnap)
    assert rel(dz, [closed(base["zl"][p]) / closed(zsnap[p]) for p in range(10)]) <= 1e-8
    # planes cut at their own snapshot redshift need no correction where zl happens to equal it: g(zl, zl) = 1
    same = slicer_amd.plane_weights(0.3, 0.7, -1.0, 5.0, 64, ld, ld2, base["zl"])
    assert rel(same["c"][live], off["c"][live]) <= 1e-12


def test_refusals():
    ld, ld2, zs = [0.0, 50.0], [50.0, 100.0], [0.0, 0.0]
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_weights(0.3, 0.6, -1.0, 2.0, 32, ld, ld2, zs)   # curved
    assert e.value.code == slicer_amd.api.ERR_UNSUPPORTED and "flat" in str(e.value)
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_weights(0.3, 0.7, -1.0, 2.0, 32, ld, ld2, zs, physical=True)
    assert e.value.code == slicer_amd.api.ERR_UNSUPPORTED
    with pytest.raises(SlicerError) as e:
        slicer_amd.plane_weights(0.3, 0.7, -1.0, 2.0, 32, [50.0, 100.0], [50.0, 150.0], zs)   # empty plane
    assert e.value.code == 2
    slicer_amd.plane_weights(0.3, 0.7 + 5e-6, -1.0, 2.0, 32, ld, ld2, zs)   # flat within 1e-5 is accepted


def test_driver_refuses_kappa_where_the_contract_does_not_hold(tmp_path):
    ini, _, out = make_cone(tmp_path, npix=-150)   # a physical pixel size: one map size per plane
    r = run([ini, "--kappa", "all"])
    assert r.returncode != 0 and "physical" in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits")]
    ini2, _, _ = make_cone(tmp_path / "bad", npix=32)
    r = run([ini2, "--kappa", "0.1,abc"])
    assert r.returncode == 2
