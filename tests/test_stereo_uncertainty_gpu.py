"""Mapping the row and depth uncertainty of a calibrated stereo pair on the device (vc_stereo_uncertainty*,
vicalib_amd/csrc/vc_stereo_uncertainty.hip): the kernels against the numpy reference and the checks of tests/stereo_uncertainty_cases.py (the ones
tests/test_stereo_uncertainty_cpu.py applies to the host build of the same arithmetic), the semantic pin against a real Rectifier built at the
perturbed calibration, the exact properties, a calibrator's pair, argument errors of a run, and the command line."""
import os
import subprocess

import numpy as np
import pytest

import stereo_uncertainty_cases as su
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Rectifier, StereoUncertainty, ViCalibrator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def read(u):
    """the last run of a handle in the layout the checks take"""
    var, fl = u.map()
    n = var.shape[0]
    return dict(var=var.reshape(n, -1, 3), flags=fl.reshape(n, -1), summary=u.summary(), pose_var=u.pose_sigma(), W=u.geometry()["W"])


def run_on(u, cov, sigma_px, depths):
    return read(u.run(cov, sigma_px, depths))


def handle(c, cameras=None, T_ck=None, dl=su.DST_LINEAR):
    (a, b), T = (cameras or c.cameras), (T_ck or c.T_ck)
    return StereoUncertainty(a, b, su.SIZE, su.SIZE, T[0], T[1], dst_size=su.SIZE, dst_linear=dl, grid=c.grid)


@pytest.mark.parametrize("name", su.case_names())
def test_cases_against_numpy(name):
    """checks 1 and 2, then the same bits from a second run of the handle and from a second handle"""
    c = su.case(name)
    u = handle(c)
    first, _ = su.check_case(name, lambda case, cov, s, depths: run_on(u, cov, s, depths))
    g = u.geometry()
    ref = su.reference(name)
    assert np.abs(g["R_ds_a"] - ref.Ra).max() <= 1e-12 and np.abs(g["R_ds_b"] - ref.Rb).max() <= 1e-12 and abs(g["baseline"] - ref.b) <= 1e-12
    assert np.array_equal(g["dst_linear"], su.DST_LINEAR) and np.array_equal(g["W"], StereoUncertainty.pose_jacobian(*c.T_ck))
    assert su.same_bits(first, run_on(u, c.cov, c.sigma_px, c.depths)) and su.same_bits(first, run_on(handle(c), c.cov, c.sigma_px, c.depths))


@pytest.mark.parametrize("what,k,delta,tab_dv,tab_d", su.PIN)
def test_rank_one_covariance_is_the_rectifiers_shift(what, k, delta, tab_dv, tab_d):
    """check 3 with |dv| and |d - d0| from a real Rectifier built at the perturbed calibration with the same dst_linear, fed the pixels the
    nominal calibration sees the samples at"""
    c, ref = su.case("%s-%s" % su.PIN_PAIR), su.reference("%s-%s" % su.PIN_PAIR)
    K, T, cov = su.pin_perturbed(what, k, delta)
    rect = Rectifier((c.models[0], K[0], su.SIZE, T[0]), (c.models[1], K[1], su.SIZE, T[1]), dst_size=su.SIZE, dst_linear=su.DST_LINEAR)
    planes = []
    for i, Z in enumerate(ref.depths):
        v = ref.valid[i] & ~ref.undecided[i]
        got = rect.check([0, int(v.sum())], ref.pix[i][0][v], ref.pix[i][1][v])
        dv, dd, use = np.full(len(v), np.nan), np.full(len(v), np.nan), v.copy()
        dv[v], dd[v] = np.abs(got["pairs"][:, 0]), np.abs(got["pairs"][:, 1] - su.DST_LINEAR[0] * ref.b / Z)
        use[v] = ~got["invalid"]
        assert use.sum() >= 0.9 * v.sum()
        planes.append((dv, dd, use))
    su.check_pin(what, k, delta, (tab_dv, tab_d), run_on(handle(c), cov, 1.0, c.depths), planes)


def test_exact_properties():
    """check 4"""
    c = su.case("kb4-poly3")
    u = handle(c)
    one = run_on(u, c.cov, 1.0, c.depths)
    zero = run_on(u, np.zeros_like(c.cov), 1.0, c.depths)
    good = (one["flags"] & su.FLAG_INVALID) == 0
    assert not np.any(zero["var"][good]) and np.array_equal(zero["flags"], one["flags"]) and not np.any(zero["pose_var"])
    assert all(s["sum_var_dv"] == 0 and s["sum_var_d"] == 0 and s["sum_var_z"] == 0 and s["max_var_dv"] == 0 for s in zero["summary"])
    assert su.same_bits(one, run_on(u, c.cov, 2.0, c.depths), scale=4.0)
    assert su.same_bits(one, run_on(u, c.cov, 1.0, c.depths)) and su.same_bits(one, run_on(handle(c), c.cov, 1.0, c.depths))
    # a depth plane alone, on the same handle and on a fresh one, and the planes in another order
    for k, Z in enumerate(c.depths):
        assert su.same_bits(su.plane(one, k), run_on(u, c.cov, 1.0, (Z,))) and su.same_bits(su.plane(one, k), run_on(handle(c), c.cov, 1.0, (Z,)))
    back = run_on(u, c.cov, 1.0, c.depths[::-1])
    for k in range(len(c.depths)):
        assert su.same_bits(su.plane(one, k), su.plane(back, len(c.depths) - 1 - k))
    eight = run_on(u, c.cov, 1.0, (c.depths[1],) * 8)
    assert all(su.same_bits(su.plane(one, 1), su.plane(eight, k)) for k in range(8))


def test_swapping_the_sides_keeps_the_row_variance():
    c = su.case("kb4-poly3")
    one = run_on(handle(c), c.cov, 1.0, c.depths)
    for k, Z in enumerate(c.depths):
        cams, T, dl, cov = su.swapped(c, Z)
        other = run_on(handle(c, cams, T, dl), cov, 1.0, (Z,))
        und = su.reference(c.name).undecided[k]
        fa, fb = one["flags"][k], other["flags"][0]
        assert np.array_equal(((fa & 1) << 1 | (fa & 2) >> 1 | (fa & 4))[~und], fb[~und])
        both = ((fa | fb) & su.FLAG_INVALID) == 0
        off = np.abs(other["var"][0][both, 0] - one["var"][k][both, 0]) / one["var"][k][both, 0]
        print("depth %g: var_dv of the swapped pair off by %.3g" % (Z, off.max()))
        assert both.sum() > 0.3 * len(both) and off.max() <= su.TOLERANCE


def test_readers_before_a_run_errors_and_timing():
    c = su.case("kb4-poly3")
    u = handle(c)
    for read_it in (u.map, u.summary, u.pose_sigma, u.time):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            read_it()
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        u.run(None, 1.0, c.depths)                                # no calibrator's covariance on this handle
    u.run(c.cov, 1.0, c.depths)
    bad_sym = c.cov.copy(); bad_sym[1, 20] += 1e-9 * c.cov.diagonal().max()
    bad_neg = c.cov.copy(); bad_neg[3, 3] = -1e-9
    bad_nan = c.cov.copy(); bad_nan[2, 5] = bad_nan[5, 2] = np.nan
    for kw in (dict(cov=bad_sym), dict(cov=bad_neg), dict(cov=bad_nan), dict(cov=c.cov, sigma_px=0.0), dict(cov=c.cov, sigma_px=float("nan")),
               dict(cov=c.cov, depths=(1.0, 0.0)), dict(cov=c.cov, depths=(float("inf"),)), dict(cov=c.cov, depths=()), dict(cov=c.cov, depths=(1.0,) * 9)):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            u.run(**kw)
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            u.summary(0)                                          # a refused run leaves nothing to read
        u.run(c.cov, 1.0, c.depths)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        u.summary(len(c.depths))
    assert (u.time(2) > 0).all()
    # the destination camera fitted instead of given: the rectifier's own
    fitted = StereoUncertainty(c.cameras[0], c.cameras[1], su.SIZE, su.SIZE, c.T_ck[0], c.T_ck[1], alpha=0.0, grid=c.grid)
    rect = Rectifier((c.models[0], c.K[0], su.SIZE, c.T_ck[0]), (c.models[1], c.K[1], su.SIZE, c.T_ck[1]), alpha=0.0)
    assert np.array_equal(fitted.geometry()["dst_linear"], rect.get()["dst_linear"])


# ---------------------------------------------------------------------------------------------------------------- a calibrator's pair
def _calibrator(prob, copies=1):
    """a vision-only calibrator at the problem's ground truth, every frame added `copies` times; no solve"""
    cal = ViCalibrator(0)
    for c in range(len(prob.cam_model)):
        cal.AddCamera(prob.cam_model[c], prob.cam_K_gt[c], prob.cam_T_ck_gt[c], prob.cfg.width, prob.cfg.height)
    n = len(prob.frame_time)
    for rep in range(copies):
        for f in range(n):
            cal.AddFrame(prob.frame_T_wk_gt[f], prob.frame_time[f] + rep * (prob.frame_time[-1] + 1.0))
    for rep in range(copies):
        for (f, c, ids, pix) in prob.tiles:
            cal.AddObservations(rep * n + f, c, prob.grid_points[ids], pix)
    cal.SetCalibrateImu(False)
    return cal


def test_for_cameras_of_a_calibrator():
    """check 5"""
    prob = synth.generate(synth.Config(models=("fov", "fov"), n_frames=12, seed=3))
    size = (prob.cfg.width, prob.cfg.height)
    cal = _calibrator(prob)
    cal.Solve()
    depths = (0.5, 2.0)
    mine = StereoUncertainty.for_cameras(cal, 0, 1, size, grid=su.GRID)
    got = run_on(mine, None, 0.1, depths)
    cov, names = cal.GetSolutionCovariance()
    assert names == ["c[0].q_ck:(4)", "c[0].p_ck:(3)", "c[0].params:(5)", "c[1].q_ck:(4)", "c[1].p_ck:(3)", "c[1].params:(5)"] and cov.shape == (24, 24)
    (Ka, Ta), (Kb, Tb) = cal.GetCamera(0), cal.GetCamera(1)
    alone = StereoUncertainty(("fov", Ka), ("fov", Kb), size, size, Ta, Tb, dst_linear=mine.geometry()["dst_linear"], grid=su.GRID)
    assert su.same_bits(got, run_on(alone, cov, 0.1, depths))
    assert all(s["count"] > 0.3 * su.GRID[0] * su.GRID[1] and s["max_var_dv"] > 0 for s in got["summary"])
    for a, b in ((0, 0), (0, 2), (-1, 1)):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            StereoUncertainty.for_cameras(cal, a, b, size, grid=su.GRID)
    # every frame twice: twice the information, half the covariance (1e-5: the rounding of S is amplified by the inverse, as in the covariance's
    # own parity test).  The doubled cost has the same minimum, so the second solve ends at the same calibration.
    two = _calibrator(prob, 2)
    two.Solve()
    twice = run_on(StereoUncertainty.for_cameras(two, 0, 1, size, dst_linear=mine.geometry()["dst_linear"], grid=su.GRID), None, 0.1, depths)
    both = ((got["flags"] | twice["flags"]) & su.FLAG_INVALID) == 0
    off = np.abs(2.0 * twice["var"][both] - got["var"][both]) / got["var"][both]
    print("every frame twice: triples halve to %.3g" % off.max())
    assert off.max() <= 1e-5
    cal.FixCameraIntrinsics(True)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        StereoUncertainty.for_cameras(cal, 0, 1, size, grid=su.GRID)


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_cli_stereo_uncertainty_dir(tmp_path):
    """check 7: a small vision-only solve of a pair with -stereo_uncertainty_dir: the files exist with one row per lattice sample and depth, and the
    rows are those of a library run on the cameras, the covariance and the noise the summary states"""
    prob = synth.generate(synth.Config(models=("fov", "fov"), n_frames=12, seed=3))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    result, out = tmp_path / "cameras.xml", tmp_path / "su"
    depths = (0.5, 2.0, 5.0)
    r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "fov,fov", "-nocalibrate_imu", "-output", str(result), "-stereo_uncertainty_dir", str(out),
                        "-stereo_uncertainty_grid", "%dx%d" % su.GRID, "-stereo_uncertainty_depths", ",".join("%g" % z for z in depths)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    n = su.GRID[0] * su.GRID[1]
    rows = np.loadtxt(out / "stereo_uncertainty.csv", delimiter=",", skiprows=1)
    assert open(out / "stereo_uncertainty.csv").readline().strip() == "depth,x,y,sigma_dv,sigma_d,sigma_Z,flags" and rows.shape == (n * len(depths), 7)
    summary = open(out / "stereo_uncertainty_summary.csv").read().splitlines()
    nd = len(depths)
    assert summary[0] == "depth,count,invalid,rms_sigma_dv,max_sigma_dv,worst_x,worst_y,rms_sigma_d,rms_sigma_z_over_z"
    assert summary[nd + 1] == "baseline,sigma_baseline,noise_px,fu,fv,u0,v0,width,height" and summary[nd + 3] == "camera,qx,qy,qz,qw,tx,ty,tz,params"
    assert summary[nd + 6] == "row,covariance" and len(summary) == nd + 7 + 24
    num = lambda ln: np.array([float(x) for x in ln.split(",")])      # noqa: E731
    per_depth = np.stack([num(ln) for ln in summary[1:nd + 1]])
    baseline, sigma_b, noise, fu, fv, u0, v0, w, h = num(summary[nd + 2])
    cams = [num(summary[nd + 4]), num(summary[nd + 5])]
    cov = np.stack([num(ln)[1:] for ln in summary[nd + 7:]])
    size = (int(w), int(h))
    assert size == (prob.cfg.width, prob.cfg.height) and cams[0][0] == 0 and cams[1][0] == 1
    u = StereoUncertainty(("fov", cams[0][8:]), ("fov", cams[1][8:]), size, size, cams[0][1:8], cams[1][1:8], dst_linear=[fu, fv, u0, v0], grid=su.GRID)
    want = run_on(u, cov, noise, depths)
    sig = np.sqrt(np.maximum(want["var"], 0.0)).reshape(-1, 3)
    assert np.array_equal(rows[:, 3:6], sig, equal_nan=True) and np.array_equal(rows[:, 6], want["flags"].ravel()) and np.array_equal(rows[:, 0], np.repeat(depths, n))
    assert abs(baseline - u.geometry()["baseline"]) == 0 and sigma_b == np.sqrt(want["pose_var"][6])
    for k, s in enumerate(want["summary"]):
        assert per_depth[k, 1] == s["count"] and per_depth[k, 2] == s["invalid"] and per_depth[k, 4] == np.sqrt(s["max_var_dv"])
        assert abs(per_depth[k, 3] - np.sqrt(s["sum_var_dv"] / s["count"])) <= 1e-15 * per_depth[k, 3]
        assert abs(per_depth[k, 8] - np.sqrt(s["sum_var_z"] / s["count"]) / depths[k]) <= 1e-15 * per_depth[k, 8]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("cameras 0,1 at ")]
    assert len(lines) == nd
