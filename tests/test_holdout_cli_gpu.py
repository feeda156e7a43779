"""The command line's -holdout_every: every Nth frame is kept out of the calibration and scored afterwards (vc_holdout_*)."""
import csv
import os
import re
import subprocess

import numpy as np
import pytest

from vicalib_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
HELD = [3, 7, 11, 15, 19, 23]


def _run(args, cwd):
    return subprocess.run([BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def _check_outputs(r, rep, p, sigma):
    assert r.returncode == 0, r.stdout + r.stderr
    # the solve saw the 18 other frames
    fitted = sorted({int(v["frame"]) for v in _rows(os.path.join(rep, "views.csv"))})
    assert fitted == [f for f in range(24) if f not in HELD]
    assert "18 frames" in r.stderr
    views = _rows(os.path.join(rep, "holdout_views.csv"))
    assert list(views[0].keys()) == ["frame", "camera", "corners", "rmse_px", "max_px", "status", "iterations"]
    assert [int(v["frame"]) for v in views] == HELD and all(v["camera"] == "0" for v in views)
    assert all(v["status"] in ("converged", "max_iters") for v in views)
    want = {f: len(ids) for (f, c, ids, px) in p.tiles}
    assert [int(v["corners"]) for v in views] == [want[f] for f in HELD]
    corners = _rows(os.path.join(rep, "holdout_corners.csv"))
    assert list(corners[0].keys()) == ["frame", "camera", "dot", "u", "v", "ru", "rv"]
    assert len(corners) == sum(want[f] for f in HELD) and sorted({int(c["frame"]) for c in corners}) == HELD
    # a view's row is the sum over its corner rows (10 digits are written)
    for v in views:
        rr = np.array([[float(c["ru"]), float(c["rv"])] for c in corners if c["frame"] == v["frame"]])
        assert abs(np.sqrt((rr ** 2).sum() / (2.0 * len(rr))) - float(v["rmse_px"])) <= 1e-8 * float(v["rmse_px"])
    # the printed held-out RMSE is the files'
    m = re.search(r"Camera 0: fitted RMSE ([-0-9.e+]+) px, held-out RMSE ([-0-9.e+]+) px over (\d+) views, (\d+) corners", r.stdout)
    assert m, r.stdout
    n = np.array([int(v["corners"]) for v in views]); e = np.array([float(v["rmse_px"]) for v in views])
    rmse = np.sqrt((e ** 2 * 2 * n).sum() / (2.0 * n.sum()))
    assert int(m.group(3)) == 6 and int(m.group(4)) == n.sum()
    assert abs(float(m.group(2)) - rmse) <= 2e-6 * rmse                 # (%.6g)
    fit = re.search(r"reprojection RMSE: ([-0-9.e+]+) px", r.stdout)
    assert float(m.group(1)) == float(fit.group(1))
    assert re.search(r"held-out frames: 6 \(every 4\.\): \d+ converged", r.stdout)
    # held-out residuals of the right model are detection noise: sigma sqrt(1 - 6 F / (2 M)) plus what the camera's own error adds
    assert rmse <= 1.5 * sigma


def test_holdout_every_vision_only(tmp_path):
    p = synth.generate(synth.Config(models=("poly3",), n_frames=24, seed=7, pixel_sigma=0.1))
    files, _ = synth.write_dataset(p, str(tmp_path))
    rep = str(tmp_path / "rep")
    r = _run(["-cam", "detections://" + files[0], "-models", "poly3", "-holdout_every", "4", "-report_dir", rep, "-output", str(tmp_path / "cameras.xml")], str(tmp_path))
    _check_outputs(r, rep, p, 0.1)
    # without the flag nothing of it is printed or written
    rep2 = str(tmp_path / "rep2")
    r2 = _run(["-cam", "detections://" + files[0], "-models", "poly3", "-report_dir", rep2, "-output", str(tmp_path / "cameras2.xml")], str(tmp_path))
    assert r2.returncode == 0 and "held-out" not in r2.stdout and not os.path.exists(os.path.join(rep2, "holdout_views.csv"))
    assert len({int(v["frame"]) for v in _rows(os.path.join(rep2, "views.csv"))}) == 24


def test_holdout_every_with_the_imu(tmp_path):
    p = synth.generate(synth.Config(models=("poly3",), n_frames=24, imu=True, seed=7, pixel_sigma=0.1))
    files, imu_dir = synth.write_dataset(p, str(tmp_path))
    rep = str(tmp_path / "rep")
    r = _run(["-cam", "detections://" + files[0], "-imu", "csv://" + imu_dir, "-models", "poly3", "-max_iters", "100", "-max_reprojection_error", "1.0", "-holdout_every", "4",
              "-report_dir", rep, "-output", str(tmp_path / "cameras.xml")], str(tmp_path))
    _check_outputs(r, rep, p, 0.1)
    assert len(_rows(os.path.join(rep, "imu_blocks.csv"))) == 17          # the IMU blocks span the gaps the held-out frames leave


def test_holdout_every_of_one_is_a_flag_error(tmp_path):
    p = synth.generate(synth.Config(models=("poly3",), n_frames=4, seed=7))
    files, _ = synth.write_dataset(p, str(tmp_path))
    r = _run(["-cam", "detections://" + files[0], "-models", "poly3", "-holdout_every", "1"], str(tmp_path))
    assert r.returncode == 1 and "illegal value '1' specified for flag 'holdout_every'" in r.stderr
