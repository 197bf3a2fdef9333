"""SLICER_amd --kappa ... --raytrace: the six ray-traced files of every source against the same
chain run through the Python API on the run's own plane files: plane_strengths -> one-source Kappa -> Shear -> Rays."""
import json
import math
import os

import numpy as np
import pytest

import slicer_amd
from test_driver import make_cone, run
from test_driver_shear import clear, files, read_fits

ANGLE = 2.0  # make_cone's fov
RT = (".rt_kappa_z", ".rt_gamma1_z", ".rt_gamma2_z", ".rt_omega_z", ".rt_alpha1_z", ".rt_alpha2_z")  # RAYS_* order
OTHERS = (".plane_", ".kappa_z", ".phi_z", ".gamma1_z", ".gamma2_z", ".gamma_z", ".alpha1_z", ".alpha2_z")


def snapshot(out, tokens):
    return {t: files(out, t) for t in tokens}


def python_chain(out, plan_path, npix, zs, gradient):
    """{(token, "%.4f" % z): f32 map} of the chain on the plane files in `out`; growth off, so that the planes_list's
    six-digit snapshot redshifts do not enter (the plan file carries ld and ld2 to the last bit)."""
    plan = json.load(open(plan_path))["planes"]
    ld, ld2 = [p["ld"] for p in plan], [p["ld2"] for p in plan]
    rows = [ln.split() for ln in open(os.path.join(out, "cone_planes_list_t0.txt")).read().strip().split("\n")]
    zsnap = [float(r[6]) for r in rows]
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    assert len(planes) == len(plan) >= 20
    ps = slicer_amd.plane_strengths(0.3, 0.7, -1.0, ANGLE, npix, ld, ld2, zsnap, sources=zs, growth=False)
    d = ANGLE * math.pi / 180.0 / npix
    got = {}

    def observe(rays, done):
        for s in np.argsort(ps["zs"], kind="stable"):
            if ps["n_in_front"][s] == done:
                o = rays.observe(ps["chis"][s])
                for k, token in enumerate(RT):
                    got[token, "%.4f" % ps["zs"][s]] = o[k]

    with slicer_amd.Slicer(0) as s, slicer_amd.Kappa(s, npix, 1) as lens, slicer_amd.Shear(s, npix, ANGLE) as sh, \
            slicer_amd.Rays(s, npix, d) as rays:
        observe(rays, 0)
        for p, name in enumerate(planes):
            dm = s.to_device(read_fits(os.path.join(out, name), npix)[1])
            lens.add_device([dm], [[ps["strength"][p]]])
            sh.run_kappa(lens, 0)
            if gradient:
                sh.fd()
            else:
                sh.deflection()
            rays.step_shear(sh, ps["chil"][p], gradient=gradient)
            lens.reset()
            observe(rays, p + 1)
            s.synchronize()
            s.free(dm)
    return got, ps


def check_rt_files(out, npix, got):
    n = 0
    for (token, z), ref in got.items():
        name = f"cone_gadget{token}{z}_{npix}_t0.fits"
        hdr, m = read_fits(os.path.join(out, name), npix)
        khdr, _ = read_fits(os.path.join(out, name.replace(token, ".kappa_z")), npix)
        assert hdr == khdr, name
        assert np.array_equal(m.view(np.uint32), ref.view(np.uint32)), name
        n += 1
    assert n == sum(len(files(out, t)) for t in RT)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("npix,derivative", [(32, "fft"), (30, "fft"), (45, "fft"), (32, "gradient"), (30, "gradient"),
                                             (45, "gradient")])
def test_rt_files_equal_the_python_chain(tmp_path, npix, derivative):
    ini, _, out = make_cone(tmp_path, npix=npix)
    plan = str(tmp_path / "plan.json")
    zs = [0.2, 0.0004, 0.05, 0.12]  # not in order; 0.0004 has no plane in front
    args = [ini, "--ngp", "--kappa", ",".join(str(z) for z in zs), "--kappa-no-growth", "--raytrace", "--dump-plan", plan]
    if derivative == "gradient":
        args += ["--shear-derivative", "gradient"]
    r = run(args)
    assert r.returncode == 0, r.stderr[-2000:]
    got, ps = python_chain(out, plan, npix, zs, derivative == "gradient")
    assert ps["n_in_front"][1] == 0 and ps["n_in_front"][0] > ps["n_in_front"][3] > ps["n_in_front"][2] > 1
    assert check_rt_files(out, npix, got) == 6 * len(zs)
    for token in RT:  # the source in front of every plane: zeros
        _, m = read_fits(os.path.join(out, f"cone_gadget{token}0.0004_{npix}_t0.fits"), npix)
        assert np.all(m == 0)
    _, far = read_fits(os.path.join(out, f"cone_gadget.rt_omega_z0.2000_{npix}_t0.fits"), npix)
    assert np.abs(far).max() > 0  # lens-lens coupling: many planes rotate
    assert not any(files(out, t) for t in OTHERS[2:])  # no --shear, no --deflection: none of their files


@pytest.mark.gpu
def test_one_plane_in_front_is_the_born_map(tmp_path):
    """With --kappa all the first source has one plane in front: A = I - w_s U there, and c_s1 = strength_1 w_s, so the
    ray-traced kappa is the Born file's up to the three f32 roundings between them (the lens map, the Born map, the
    ray-traced map) and the f64 ones, and the rotation is exactly zero."""
    npix = 32
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini, "--ngp", "--kappa", "all", "--raytrace"])
    assert r.returncode == 0, r.stderr[-2000:]
    kap = sorted(files(out, ".kappa_z"))
    assert len(kap) >= 20 and all(len(files(out, t)) == len(kap) for t in RT)
    _, born = read_fits(os.path.join(out, kap[0]), npix)
    _, rt = read_fits(os.path.join(out, kap[0].replace(".kappa_z", ".rt_kappa_z")), npix)
    _, om = read_fits(os.path.join(out, kap[0].replace(".kappa_z", ".rt_omega_z")), npix)
    b = born.astype(np.float64)
    assert np.all(np.abs(rt - b) <= 3 * 2.0 ** -24 * np.abs(b) + 2.0 ** -50)
    assert np.all(om == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("derivative", ["fft", "gradient"])
def test_every_other_file_is_the_same_with_and_without_raytrace(tmp_path, derivative):
    ini, _, out = make_cone(tmp_path)
    base = [ini, "--ngp", "--kappa", "all", "--shear", "--deflection", "--shear-derivative", derivative]
    r = run(base)
    assert r.returncode == 0, r.stderr[-2000:]
    without = snapshot(out, OTHERS)
    assert all(without[t] for t in OTHERS) and not any(files(out, t) for t in RT)
    clear(out)
    r = run(base + ["--raytrace"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert snapshot(out, OTHERS) == without
    assert all(len(files(out, t)) == len(without[".kappa_z"]) for t in RT)


@pytest.mark.gpu
def test_resumed_two_rank_and_reordered_runs_give_the_same_files(tmp_path):
    ini, _, out = make_cone(tmp_path)
    args = ["--accum", "fixed64", "--kappa", "0.05,0.1,0.2", "--raytrace"]
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    one = snapshot(out, RT)
    assert sorted(one[".rt_omega_z"]) == ["cone_gadget.rt_omega_z0.0500_32_t0.fits", "cone_gadget.rt_omega_z0.1000_32_t0.fits",
                                          "cone_gadget.rt_omega_z0.2000_32_t0.fits"]
    # resume: some plane files removed, the others read back
    for t in RT + (".kappa_z",):
        for f in files(out, t):
            os.remove(os.path.join(out, f))
    planes = sorted(f for f in os.listdir(out) if ".plane_" in f)
    for f in planes[1::3]:
        os.remove(os.path.join(out, f))
    r = run([ini] + args)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Already exists" in r.stdout
    assert snapshot(out, RT) == one
    clear(out)
    r = run([ini] + args + ["--devices", "0,0", "--reduce", "host"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert snapshot(out, RT) == one
    clear(out)
    r = run([ini, "--accum", "fixed64", "--kappa", "0.2,0.1,0.05", "--raytrace"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert snapshot(out, RT) == one


@pytest.mark.gpu
@pytest.mark.parametrize("npix,args,text", [
    (32, ["--raytrace"], "--raytrace needs --kappa"),
    (32, ["--shear", "--raytrace"], "needs --kappa"),
    (37, ["--kappa", "all", "--raytrace"], "--raytrace: npix = 37"),
    (4, ["--kappa", "all", "--raytrace", "--shear-derivative", "gradient"], "npix = 4"),
    (32, ["--kappa", "all", "--raytrace", "--shear-derivative", "stencil"], "bad --shear-derivative"),
    (-150, ["--kappa", "all", "--raytrace"], "physical"),
])
def test_bad_requests_are_refused_before_any_plane(tmp_path, npix, args, text):
    ini, _, out = make_cone(tmp_path, npix=npix)
    r = run([ini] + args)
    assert r.returncode != 0
    assert text in r.stderr
    assert not [f for f in os.listdir(out) if f.endswith(".fits")]
