"""-dot_bias_rounds end to end, the test that fails without the feature: the command line calibrates the case of tests/dot_bias_cli_case.py (a
`linear` camera, 20 views of the 9 x 6 board, the measurements the exact centres of the dots' image ellipses, no noise) once as it always did
and once with two rounds of the correction.  The largest error of fx, fy, cx, cy against the truth must fall to at most 1/20 (the numpy
reference's own experiment gives a factor above 1000 after ONE round; the margin leaves room for the LM's -function_tolerance 1e-6 stop), the
RMSE must fall, and -dot_bias_rounds 0 must print what the command prints without the new flags.

Measured (MI355X): see DESIGN 4.20."""
import os
import re
import subprocess

import numpy as np
import pytest

import dot_bias_cli_case as case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
RADII = ["-grid_large_rad", "0.0094", "-grid_small_rad", "0.0063"]


def _run(tmp_path, name, extra):
    det, pat = case.write(str(tmp_path))
    out = tmp_path / (name + ".xml")
    args = [BIN, "-cam", "detections://" + det, "-models", "linear", "-nocalibrate_imu", "-grid_width", "9", "-grid_height", "6", "-image_width", "640",
            "-image_height", "480", "-output", str(out)] + extra
    r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 2), r.stdout + r.stderr
    params = np.array([float(x) for x in re.search(r"<params>\s*\[(.*?)\]", open(out).read(), re.S).group(1).split(";")])
    rmse = float(re.search(r"reprojection RMSE: ([0-9.eE+-]+) px", r.stdout).group(1))
    return r, params, rmse, open(out).read()


def _stable(r, out_name):
    """what a run prints, without what differs from run to run by itself: the solve time, the iterations the 30 ms poll happened to see, the output's name"""
    stdout = re.sub(r"solve time: [0-9.]+ s", "solve time: - s", r.stdout).replace(out_name, "OUT")
    stderr = "\n".join(l for l in r.stderr.splitlines() if not l.startswith("I iteration ")).replace(out_name, "OUT")
    return stdout, stderr


def test_two_rounds_remove_the_bias_from_the_calibration(tmp_path):
    ref_case = case.build()                                  # (asserts the reference's own factor of at least 100 after one round)
    pattern = ["-grid_pattern_file", str(tmp_path / "pattern.txt")]
    plain, k_plain, rmse_plain, xml_plain = _run(tmp_path, "plain", [])
    zero, k_zero, rmse_zero, xml_zero = _run(tmp_path, "zero", ["-dot_bias_rounds", "0", "-dot_radius", "0.005"] + RADII)
    two, k_two, rmse_two, _ = _run(tmp_path, "two", ["-dot_bias_rounds", "2"] + pattern + RADII)
    print(two.stderr[-2500:])
    err_plain, err_two = np.abs(k_plain[:4] - case.K_TRUE).max(), np.abs(k_two[:4] - case.K_TRUE).max()
    print("errors of fx fy cx cy: without %s (largest %.3e px), with two rounds %s (largest %.3e px), ratio %.1f; RMSE %.3e -> %.3e px; reference: %.3e -> %.3e px after one round"
          % (k_plain[:4] - case.K_TRUE, err_plain, k_two[:4] - case.K_TRUE, err_two, err_plain / err_two, rmse_plain, rmse_two, ref_case["err0"], ref_case["err1"]))
    # N = 0 is today's tool, byte for byte
    assert _stable(zero, "zero.xml") == _stable(plain, "plain.xml")
    assert xml_zero == xml_plain and "dot bias" not in zero.stderr
    # the rounds ran and say so
    lines = re.findall(r"I dot bias round (\d), camera 0: bias rms ([0-9.]+) px, max ([0-9.]+) px over (\d+) observations, (\d+) without a prediction, RMSE (\S+) -> (\S+) px", two.stderr)
    assert [l[0] for l in lines] == ["1", "2"] and all(l[3] == "1080" and l[4] == "0" for l in lines), two.stderr
    assert abs(float(lines[0][1]) - ref_case["bias_rms"]) < 2e-3 and abs(float(lines[0][2]) - ref_case["bias_max"]) < 5e-3, (lines[0], ref_case["bias_rms"], ref_case["bias_max"])
    assert "W dot bias" not in two.stderr
    # the yardstick
    assert err_two <= err_plain / 20.0, (err_plain, err_two)
    assert rmse_two < rmse_plain, (rmse_plain, rmse_two)
    assert two.returncode == 0 and "calibration succeeded" in two.stdout


def test_the_table_of_the_last_round(tmp_path):
    """-report_dir gets dot_bias.csv: one row per calibrated observation, status 0, a bias of the size the reference predicts; -dot_radius gives every
    dot one radius"""
    report = tmp_path / "report"
    r, _, _, _ = _run(tmp_path, "one", ["-dot_bias_rounds", "1", "-dot_radius", "0.0094", "-report_dir", str(report)])
    rows = np.loadtxt(report / "dot_bias.csv", delimiter=",", skiprows=1)
    assert open(report / "dot_bias.csv").readline().strip() == "frame,camera,dot,bu,bv,radius_px,status"
    assert rows.shape == (1080, 7) and (rows[:, 6] == 0).all() and (rows[:, 1] == 0).all()
    assert sorted(set(rows[:, 0])) == list(range(20)) and sorted(set(rows[:, 2])) == list(range(54))
    assert 5.0 < rows[:, 5].min() and rows[:, 5].max() < 13.0                     # 9.4 mm at 0.35 to 0.55 m and f = 420: 7 to 11 px, tilted
    assert 0.02 < np.sqrt(np.mean(rows[:, 3] ** 2 + rows[:, 4] ** 2)) < 0.2
    assert os.path.exists(report / "corners.csv")
