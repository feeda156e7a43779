"""The batched planar PnP on the device (vc_pnp_planar_batch, one wavefront per view) against the host routine it stands in for, on the views of
tests/seed_cases.py with that file's checks: the project's parameter tolerances (rotation 1e-6 rad, translation 1e-6 relative floored at
1e-9 m, rms 1e-6 relative floored at 1e-9 px), the inlier mask exactly, the statuses of the refusals, the outputs of a refused view untouched.
Determinism is compared with == on the raw doubles: a fixed reduction order promises the same bits for a view alone, among others and on a
second run.  Then the three places the switch of vc_set_pnp_device reaches: vc_init_frame_poses_pnp, the seeds of vc_holdout_compute, the
command line's -pnp_device."""
import os
import re
import subprocess

import numpy as np
import pytest

import seed_cases as sc
from vicalib_amd import synth
from vicalib_amd.lib import ViCalibrator, pnp_planar_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
NO_SEED = 3          # vc_holdout_frames: no view of the frame gave a pose


def _run_batch(views, its, tol):
    models, params, off, pw, pc = sc.batch_arrays(views)
    n = len(views)
    out = dict(T_cw=np.full((n, 7), -7.0), rms=np.full(n, -7.0), n_inliers=np.full(n, -7, dtype=np.int32))
    got = pnp_planar_batch(models, params, off, pw, pc, iterations=its, tol_px=tol, out=out)
    got["inlier"] = sc.split(off, got["inlier"])
    return got


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            g = sc.group(name)
            cache[name] = _run_batch(g["views"], g["its"], g["tol"])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sc.GROUPS)
def test_batch_matches_the_host_routine(runs, name):
    got = runs(name)
    sc.check_against_host(name, got, label=" (device)")
    for k, v in enumerate(sc.group(name)["views"]):
        if got["status"][k] != sc.OK:          # a refused view: the caller's values are still there
            assert np.all(got["T_cw"][k] == -7.0) and got["rms"][k] == -7.0 and got["n_inliers"][k] == -7 and not got["inlier"][k].any(), v["name"]


def test_refusal_statuses(runs):
    assert runs("plain")["status"][-2:].tolist() == [sc.FEW, sc.NOT_PLANAR]
    assert runs("noise")["status"].tolist() == [sc.NO_CONSENSUS, sc.OK]


def _same_bits(a, b, rows_a, rows_b):
    for ka, kb in zip(rows_a, rows_b):
        assert a["status"][ka] == b["status"][kb] and a["n_inliers"][ka] == b["n_inliers"][kb]
        assert np.array_equal(a["T_cw"][ka], b["T_cw"][kb]) and a["rms"][ka] == b["rms"][kb] and np.array_equal(a["inlier"][ka], b["inlier"][kb])


@pytest.mark.parametrize("name", ["robust", "plain"])
def test_a_view_gives_the_same_bits_alone_among_others_and_again(runs, name):
    """batches of 1, 4, 5 and 9 views: a lone wave, a full workgroup, a workgroup and one wave, two workgroups and one wave"""
    g = sc.group(name)
    views = g["views"][:9]
    nine = _run_batch(views, g["its"], g["tol"])
    _same_bits(nine, runs(name), range(9), range(9))                   # (the group's own run holds the same views first)
    _same_bits(nine, _run_batch(views, g["its"], g["tol"]), range(9), range(9))
    for size in (1, 4, 5):
        _same_bits(_run_batch(views[:size], g["its"], g["tol"]), nine, range(size), range(size))
    for k in range(9):
        _same_bits(_run_batch(views[k:k + 1], g["its"], g["tol"]), nine, [0], [k])


# ------------------------------------------------------------------------------------------------ the calibrator's switch
def _rig(mismatch):
    """two cameras, 9 frames: camera 0 has 3 corners in frames 2 and 5 (the seed comes from camera 1), frame 7 has no usable view"""
    p = synth.generate(synth.Config(models=("fov", "poly3"), n_frames=9, seed=21, pixel_sigma=0.05))
    rng = np.random.default_rng(8)
    tiles = []
    for (f, c, ids, pix) in p.tiles:
        pix = pix.copy()
        n = len(ids)
        if mismatch and n >= 8:
            bad = rng.choice(n, size=max(1, n // 5), replace=False)
            pix[bad] = pix[(bad + 2 + rng.integers(0, n - 4, size=len(bad))) % n]
        keep = 3 if (f in (2, 5) and c == 0) or f == 7 else len(ids)
        tiles.append((f, c, ids[:keep], pix[:keep]))
    assert sorted({f for (f, c, ids, pix) in tiles if len(ids) >= 4}) == [0, 1, 2, 3, 4, 5, 6, 8]
    assert all(any(t[0] == f and t[1] == 1 and len(t[2]) >= 4 for t in tiles) for f in (2, 5))
    return p, tiles


def _calibrator(p, tiles, device_seeds):
    cal = ViCalibrator(0)
    for c, m in enumerate(p.cam_model):
        cal.AddCamera(m, p.cam_K_gt[c], p.cam_T_ck_gt[c], p.cfg.width, p.cfg.height)
    for n in range(len(p.frame_time)):
        cal.AddFrame(p.frame_T_wk_init[n], p.frame_time[n])
    for (f, c, ids, pix) in tiles:
        cal.AddObservations(f, c, p.grid_points[ids], pix)
    cal.SetPnPDevice(device_seeds)
    return cal


def _check_poses(label, got, want, frames):
    worst_t = worst_r = 0.0
    for f in frames:
        dt, dr = sc.pose_distance(got[f], want[f])
        worst_t = max(worst_t, dt / max(1e-6 * np.linalg.norm(want[f][4:]), 1e-9)); worst_r = max(worst_r, dr / 1e-6)
    print("%s: worst of value / bound -- translation %.3e, rotation %.3e" % (label, worst_t, worst_r))
    assert worst_t <= 1.0 and worst_r <= 1.0


@pytest.mark.parametrize("robust", [False, True])
def test_init_frame_poses_on_the_device_matches_the_host_path(robust):
    p, tiles = _rig(mismatch=robust)
    host, dev = _calibrator(p, tiles, False), _calibrator(p, tiles, True)
    if robust:
        host.SetPnPRansac(100, 1.0); dev.SetPnPRansac(100, 1.0)
    before = dev.GetFrames()
    n_host, n_dev = host.InitFramePosesPnP(), dev.InitFramePosesPnP()
    assert n_host == 8 and n_dev == n_host
    T_host, T_dev = host.GetFrames(), dev.GetFrames()
    _check_poses("seeds%s" % (" (robust)" if robust else ""), T_dev, T_host, [0, 1, 2, 3, 4, 5, 6, 8])
    assert np.array_equal(T_dev[7], before[7]) and np.array_equal(T_host[7], before[7])      # the unseeded frame, bit for bit
    assert not np.array_equal(T_dev[2], before[2]) and not np.array_equal(T_dev[5], before[5])
    dev.SetPnPDevice(False)                                                                  # the switch off again: the host's own bits
    dev.InitFramePosesPnP()
    assert np.array_equal(dev.GetFrames(), T_host)


def test_holdout_seeds_on_the_device_match_the_host_path():
    p, tiles = _rig(mismatch=False)
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])])
    res = []
    for on in (False, True):
        cal = _calibrator(p, [], on)
        cal.SetFunctionTolerance(1e-12); cal.SetTolerances(1e-14, 1e-14)
        cal.HoldoutAddTiles([t[0] for t in tiles], [t[1] for t in tiles], off, p.grid_points, np.concatenate([t[2] for t in tiles]),
                            np.concatenate([t[3] for t in tiles]))
        res.append(cal.HoldoutCompute(None, max_iters=100)["frames"])
    assert res[0]["status"].tolist() == res[1]["status"].tolist() and res[0]["status"][7] == NO_SEED
    fitted = [f for f in range(9) if res[0]["status"][f] != NO_SEED]
    assert fitted == [0, 1, 2, 3, 4, 5, 6, 8]
    _check_poses("held-out refit from device seeds", res[1]["T_wk"], res[0]["T_wk"], fitted)


def test_cli_pnp_device(tmp_path):
    """the stereo detection-file case of test_cli_stereo_calibration_from_detection_files, seeded on the device"""
    p = synth.generate(synth.Config(models=("fov", "poly3"), n_frames=40, seed=12))
    files, _ = synth.write_dataset(p, str(tmp_path))
    seeded = []
    for extra in ([], ["-pnp_device"]):
        out = tmp_path / ("cameras%d.xml" % len(extra))
        r = subprocess.run([BIN, "-cam", "detections://" + ",".join(files), "-models", "fov,poly3", "-nocalibrate_imu", "-grid_preset", "small", "-output", str(out)] + extra,
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "calibration succeeded" in r.stdout
        seeded.append(int(re.search(r"\((\d+) with a PnP seed\)", r.stderr).group(1)))
        s = open(out).read()
        for c, block in enumerate(s.split("<camera>")[1:]):
            params = [float(x) for x in re.search(r"<params>\s*\[(.*?)\]", block, re.S).group(1).split(";")]
            np.testing.assert_allclose(params[:4], p.cam_K_gt[c][:4], rtol=3e-3)
    assert seeded[0] == seeded[1] and seeded[0] > 0
