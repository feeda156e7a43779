"""-refine_target_rounds end to end, the test that fails without the feature: the command line calibrates the case of tests/target_refine_cli_case.py (a
`linear` camera, 20 views of a bowed and mis-scaled 9 x 6 board, exact measurements, the detections naming the nominal grid) once as it always did
and once with two rounds of the target step.  The largest error of fx, fy, cx, cy against the truth must fall to at most 1/20 (the reference's
own experiment is asserted to give a factor of at least 100; the margin leaves room for the LM's -function_tolerance stop), the RMSE must fall,
the refined target must match the true board up to a similarity within 10 x the reference experiment's own shape error, a second calibration
given that file through -target_points and no rounds must meet the same 1/20, and -refine_target_rounds 0 must print what the command prints
without the new flags.

Measured (MI355X): see DESIGN 4.22."""
import os
import re
import subprocess

import numpy as np
import pytest

import target_refine_cli_case as case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def _run(tmp_path, name, extra):
    det = case.write(str(tmp_path))
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


def test_two_rounds_take_the_board_out_of_the_intrinsics(tmp_path):
    ref_case = case.build()                                  # (asserts the reference's own factor of at least 100 at the defaults)
    plain, k_plain, rmse_plain, xml_plain = _run(tmp_path, "plain", [])
    zero, k_zero, rmse_zero, xml_zero = _run(tmp_path, "zero", ["-refine_target_rounds", "0", "-refine_target_sigma", "0.02", "-refine_target_output", "never.csv"])
    two, k_two, rmse_two, _ = _run(tmp_path, "two", ["-refine_target_rounds", "2", "-refine_target_output", "board.csv"])
    print(two.stderr[-2500:])
    err_plain, err_two = np.abs(k_plain[:4] - case.K_TRUE).max(), np.abs(k_two[:4] - case.K_TRUE).max()
    # N = 0 is today's tool, byte for byte
    assert _stable(zero, "zero.xml") == _stable(plain, "plain.xml")
    assert xml_zero == xml_plain and "target round" not in zero.stderr and not os.path.exists(tmp_path / "never.csv")
    # the rounds ran and say so
    lines = re.findall(r"I target round (\d): offset rms (\S+) (\S+) (\S+) mm, max (\S+) mm, (\d+) points refined, (\d+) unobserved, gauge rank (\d), RMSE (\S+) -> (\S+) px", two.stderr)
    assert [l[0] for l in lines] == ["1", "2"] and all(l[5] == "54" and l[6] == "0" and l[7] == "7" for l in lines), two.stderr
    assert "W target round" not in two.stderr
    # the refined target against the true board, up to a similarity
    rows = np.loadtxt(tmp_path / "board.csv", delimiter=",", skiprows=1)
    assert open(tmp_path / "board.csv").readline().strip() == "dot,x,y,z,nx,ny,nz,corners,status"
    assert rows.shape == (54, 9) and (rows[:, 8] == 0).all() and (rows[:, 7] == 20).all() and np.array_equal(rows[:, 4:7], ref_case["nominal"])
    shape = case.shape_error(rows[:, 1:4], ref_case["true"])
    # a second calibration from the measured target, no rounds
    again, k_again, rmse_again, _ = _run(tmp_path, "again", ["-target_points", str(tmp_path / "board.csv")])
    err_again = np.abs(k_again[:4] - case.K_TRUE).max()
    print("errors of fx fy cx cy: without %.3e px, two rounds %.3e px (ratio %.1f), from -target_points %.3e px (ratio %.1f); RMSE %.3e -> %.3e px; shape error %.5f mm "
          "(nominal %.5f mm); reference: errors %s px, shape %.5f mm"
          % (err_plain, err_two, err_plain / err_two, err_again, err_plain / err_again, rmse_plain, rmse_two, 1e3 * shape, 1e3 * ref_case["shape"][0],
             ref_case["err"], 1e3 * ref_case["shape"][-1]))
    assert err_two <= err_plain / 20.0, (err_plain, err_two)
    assert rmse_two < rmse_plain, (rmse_plain, rmse_two)
    assert shape <= 10.0 * ref_case["shape"][-1], (shape, ref_case["shape"])
    assert err_again <= err_plain / 20.0, (err_plain, err_again)
    assert two.returncode == 0 and "calibration succeeded" in two.stdout
