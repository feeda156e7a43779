"""Mapping the projection uncertainty of a calibrated camera on the device (vc_uncertainty*, vicalib_amd/csrc/vc_uncertainty.hip): the kernels
against the numpy reference and the checks of tests/uncertainty_cases.py (the ones tests/test_uncertainty_cpu.py applies to the host build of
the same arithmetic), the semantic pin against the real Comparer, the exact properties, a calibrator's camera, argument errors of a run, and
the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import compare_cases as cc
import uncertainty_cases as un
import undistort_cases as uc
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Comparer, Uncertainty, ViCalibrator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def read(u, ring_counts=un.RING_COUNTS):
    """the last run of a handle in the layout the checks take"""
    out = u.fit()
    sg, fl = u.map()
    out.update(sigma=sg.reshape(-1, 3), flags=fl.ravel(), summary=u.summary(), rings={n: u.rings(n) for n in ring_counts})
    return out


def run_on(u, cov, sigma_px, fit_radius, ring_counts=un.RING_COUNTS):
    u.run(cov, sigma_px, fit_radius)
    return read(u, ring_counts)


def handle(c):
    return Uncertainty(c.camera, un.SIZE, c.grid)


@pytest.mark.parametrize("name", un.case_names())
def test_cases_against_numpy(name):
    """checks 1 and 2, then the same bits from a second run of the handle and from a second handle"""
    c = un.case(name)
    u = handle(c)
    first, _ = un.check_case(name, lambda case, cov, s, r: run_on(u, cov, s, r))
    assert un.same_bits(first, run_on(u, c.cov, c.sigma_px, c.fit_radius)) and un.same_bits(first, run_on(handle(c), c.cov, c.sigma_px, c.fit_radius))


@pytest.mark.parametrize("model,k,delta,tabulated", un.PIN)
def test_rank_one_covariance_is_the_comparers_difference(model, k, delta, tabulated):
    """check 3 with d and the rotation from the real Comparer of K against K + delta e_k on the same lattice, at the same fit radius"""
    K = uc.gt(model)
    Kb = K.copy(); Kb[k] += delta
    cmp = Comparer((model, K), (model, Kb), un.SIZE, un.GRID)
    fit = cmp.run(un.PIN_FIT_RADIUS)
    d, fl = cmp.map()
    assert fit["status"] == 0 and not fl.any()
    out = run_on(Uncertainty((model, K), un.SIZE, un.GRID), un.pin_cov(model, k, delta), 1.0, un.PIN_FIT_RADIUS)
    un.check_pin(model, k, delta, tabulated, out, d.reshape(-1, 2), un.rotation_vector(fit["R"]))


def test_exact_properties():
    """check 4"""
    c = un.case("kb4-0.5")
    u = handle(c)
    one = run_on(u, c.cov, 1.0, 0.5)
    zero = run_on(u, np.zeros_like(c.cov), 1.0, 0.5)
    assert not np.any(zero["sigma"]) and np.array_equal(zero["flags"], one["flags"]) and zero["summary"]["sum_var"] == 0 and zero["summary"]["max_lam"] == 0
    assert un.same_bits(one, run_on(u, c.cov, 2.0, 0.5), scale=4.0)
    # no compensation: M is zero and the triples are B Cov B^T
    ref = un.reference("kb4-0")
    plain = run_on(u, c.cov, 1.0, 0.0)
    assert not np.any(plain["M"]) and plain["n_fit"] == 0
    un.check_map(ref, c.cov, 1.0, plain, "kb4 without compensation")
    assert un.same_bits(plain, run_on(u, c.cov, 1.0, -1.0))
    # a change of the fit radius on one handle equals a fresh handle at that radius
    for radius in (1.0, 0.5, 0.0, 0.5):
        assert un.same_bits(run_on(u, c.cov, 1.0, radius), run_on(handle(c), c.cov, 1.0, radius)), radius


@pytest.mark.parametrize("grid,fit_radius", cc.BOUNDARY_LATTICES)
def test_workgroup_boundary_lattices(grid, fit_radius):
    """poly3 with its dense covariance where a sweep or the Gram sweep fills its workgroups exactly or by one or two samples more, rings at
    1, 5, 8 and 64: checks 1 and 2 and the same bits from a second run"""
    c = un.Case("boundary", "poly3", uc.gt("poly3"), fit_radius, grid=grid)
    ref = un.Reference(c.model, c.K, grid, fit_radius)
    cc.assert_thresholds_decided(ref.rho, 0.5, cc.BOUNDARY_RING_COUNTS)
    cc.assert_thresholds_decided(ref.rho, fit_radius, cc.BOUNDARY_RING_COUNTS)
    u = handle(c)
    first = run_on(u, c.cov, c.sigma_px, fit_radius, cc.BOUNDARY_RING_COUNTS)
    assert first["n_fit"] == (ref.rho <= fit_radius).sum() and first["summary"]["count"] == grid[0] * grid[1]
    un.check_map(ref, c.cov, c.sigma_px, first, "boundary %dx%d" % grid)
    un.check_sums(ref, c.cov, c.sigma_px, first)
    assert un.same_bits(first, run_on(u, c.cov, c.sigma_px, fit_radius, cc.BOUNDARY_RING_COUNTS))


def test_readers_before_a_run_errors_and_timing():
    c = un.case("poly3-1")
    u = handle(c)
    for read_it in (u.fit, u.map, u.summary, u.rings, u.time):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            read_it()
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        u.run(None, 1.0, 0.5)                                     # no calibrator's covariance on this handle
    u.run(c.cov, 1.0, 0.5)
    bad_sym = c.cov.copy(); bad_sym[1, 4] += 1e-9
    bad_neg = c.cov.copy(); bad_neg[3, 3] = -1e-6
    bad_nan = c.cov.copy(); bad_nan[2, 5] = bad_nan[5, 2] = np.nan
    for kw in (dict(cov=bad_sym), dict(cov=bad_neg), dict(cov=bad_nan), dict(cov=c.cov, sigma_px=0.0), dict(cov=c.cov, sigma_px=-1.0), dict(cov=c.cov, sigma_px=float("nan")),
               dict(cov=c.cov, sigma_px=float("inf")), dict(cov=c.cov, fit_radius=float("nan"))):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            u.run(**kw)
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            u.summary()                                           # a refused run leaves nothing to read
        u.run(c.cov, 1.0, 0.5)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        u.rings(0)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        u.rings(65)
    assert (u.time(2) > 0).all()
    # 2 x 2: the four corners are the whole fit set at radius 1; none of them is within half the half-diagonal
    tiny = Uncertainty(c.camera, un.SIZE, un.TINY)
    assert tiny.run(c.cov, 1.0, 1.0)["n_fit"] == 4 and tiny.summary()["count"] == 4
    with pytest.raises(lib.VicalibError, match="NUMERIC"):
        tiny.run(c.cov, 1.0, 0.5)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        tiny.fit()
    assert tiny.run(c.cov, 1.0, 1.0)["n_fit"] == 4


# ---------------------------------------------------------------------------------------------------------------- a calibrator's camera
def _calibrator(prob, copies=1):
    """a vision-only calibrator at the problem's ground truth, every frame added `copies` times; no solve"""
    cal = ViCalibrator(0)
    cal.AddCamera(prob.cam_model[0], prob.cam_K_gt[0], prob.cam_T_ck_gt[0], prob.cfg.width, prob.cfg.height)
    n = len(prob.frame_time)
    for rep in range(copies):
        for f in range(n):
            cal.AddFrame(prob.frame_T_wk_gt[f], prob.frame_time[f] + rep * (prob.frame_time[-1] + 1.0))
    for rep in range(copies):
        for (f, c, ids, pix) in prob.tiles:
            cal.AddObservations(rep * n + f, c, prob.grid_points[ids], pix)
    cal.SetCalibrateImu(False)
    return cal


def test_for_camera_of_a_calibrator():
    prob = synth.generate(synth.Config(models=("poly3",), n_frames=6, seed=3))
    cal = _calibrator(prob)
    mine = Uncertainty.for_camera(cal, 0, un.GRID)
    got = run_on(mine, None, 0.1, 0.5)
    cov, names = cal.GetSolutionCovariance()
    assert names == ["c[0].q_ck:(4)", "c[0].p_ck:(3)", "c[0].params:(7)"]
    K, _ = cal.GetCamera(0)
    alone = Uncertainty(("poly3", K), (prob.cfg.width, prob.cfg.height), un.GRID)
    assert un.same_bits(got, run_on(alone, cov[7:14, 7:14], 0.1, 0.5))
    assert got["summary"]["count"] == un.GRID[0] * un.GRID[1] and got["summary"]["max_lam"] > 0
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        Uncertainty.for_camera(cal, 1, un.GRID)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        Uncertainty.for_camera(cal, -1, un.GRID)
    # every frame twice: twice the information, half the covariance (1e-5 of var: the rounding of S is amplified by the inverse, as in the
    # covariance's own parity test)
    twice = run_on(Uncertainty.for_camera(_calibrator(prob, 2), 0, un.GRID), None, 0.1, 0.5)
    var = got["sigma"][:, 0] + got["sigma"][:, 2]
    off = np.abs(2.0 * twice["sigma"] - got["sigma"]).max(axis=1) / var
    print("every frame twice: triples halve to %.3g of var" % off.max())
    assert off.max() <= 1e-5
    cal.FixCameraIntrinsics(True)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        Uncertainty.for_camera(cal, 0, un.GRID)


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_cli_uncertainty_dir(tmp_path):
    """a small vision-only solve with -uncertainty_dir: the files exist with one row per lattice sample, sigma_max^2 is the lam of a library run
    on the written camera with the covariance and the noise the summary states, and that noise is the camera's reprojection RMSE"""
    prob = synth.generate(synth.Config(models=("poly3",), n_frames=12, seed=3))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    result, out = tmp_path / "cameras.xml", tmp_path / "unc"
    r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "poly3", "-nocalibrate_imu", "-output", str(result), "-uncertainty_dir", str(out),
                        "-uncertainty_grid", "%dx%d" % un.GRID, "-uncertainty_rings", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n = un.GRID[0] * un.GRID[1]
    rows = np.loadtxt(out / "uncertainty_cam0.csv", delimiter=",", skiprows=1)
    assert open(out / "uncertainty_cam0.csv").readline().strip() == "x,y,s_uu,s_uv,s_vv,sigma_max,flags" and rows.shape == (n, 7)
    summary = open(out / "uncertainty_summary.csv").read().splitlines()
    assert summary[0] == "camera,ring,rho_from,rho_to,count,invalid,rms_px,max_sigma_px,noise_px" and summary[6] == "camera,parameter,covariance"
    rings = np.array([[float(x) for x in ln.split(",")] for ln in summary[1:6]])
    cov = np.array([[float(x) for x in ln.split(",")[2:]] for ln in summary[7:14]])
    noise = rings[0, 8]
    rmse = float(re.search(r"reprojection RMSE: (\S+) px", r.stdout).group(1))
    assert abs(noise - rmse) <= 1e-5 * rmse and (rings[:, 8] == noise).all()
    block = re.search(r"<params> \[(.*?)\] </params>", result.read_text()).group(1)
    K = np.array([float(x) for x in block.split(";")])
    u = Uncertainty(("poly3", K), (prob.cfg.width, prob.cfg.height), un.GRID)
    want = run_on(u, cov, noise, 0.5, ring_counts=(5,))
    assert np.array_equal(rows[:, 2:5], want["sigma"]) and np.array_equal(rows[:, 6], want["flags"])
    _, lam = un.var_lam(want["sigma"])
    assert np.abs(rows[:, 5] ** 2 - lam).max() <= 1e-15 * lam.max()
    assert np.array_equal(rings[:, 4], want["rings"][5]["count"]) and np.abs(rings[:, 7] ** 2 - want["rings"][5]["max_lam"]).max() <= 1e-15 * lam.max()
    assert np.abs(rings[:, 6] ** 2 * rings[:, 4] - want["rings"][5]["sum_var"]).max() <= 1e-14 * want["rings"][5]["sum_var"].max()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("camera 0: projection uncertainty: worst sigma_max")]
    assert len(line) == 1
    assert abs(float(line[0].split("sigma_max")[1].split()[0]) - np.sqrt(want["summary"]["max_lam"])) <= 1e-3 * np.sqrt(want["summary"]["max_lam"])
