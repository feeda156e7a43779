"""The inertial seed on the device (vc_seed_imu*: prefix integrals by block totals, a scan of the totals and blocks that scan with their carry; a
sweep over (chunk, lag) with one 18-double partial each and a finishing kernel; the gravity sums) against the numpy reference
(tests/seed_imu_ref.py), on the cases of tests/seed_imu_cases.py with that file's checks: J, the rotation, the bias, the gravity angles and
the picked offset within 100 times the spread between the reference's float64 and longdouble routes, counts, statuses and the coarse
argmin exactly, the known answers, bytes for a second run, a lag alone and the gyro channels permuted.  The refusals that need a device.
Then a calibration that starts from the seed, and the command line's -seed_imu.

Measured (MI355X): see DESIGN 4.19."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import seed_imu_cases as sc
import seed_imu_ref as ref
import vicalib_amd.lib as lib
from vicalib_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE = -2, -1
# the tolerances of tests/test_vi_sim.py (vi_sim_test.cpp:7-10) for its recovered parameters
LOGDIFF_TOLERANCE, REPROJ_TOLERANCE, CAMERA_TOLERANCE, TIMEOFFSET_TOLERANCE = 1e-3, 1e-1, 5, 1e-4
OFFSET = 0.12


@pytest.mark.parametrize("name", sc.GROUPS)
def test_device_matches_the_reference(name):
    sc.check(name, sc.DeviceSeedImu, label=" (device)")


def test_known_answers():
    sc.check_known(sc.DeviceSeedImu, " (device)")


def test_the_same_bits_again_alone_and_with_the_channels_permuted():
    sc.check_bytes(sc.DeviceSeedImu)


def test_the_device_and_the_host_build_pick_the_same_lattice_point():
    """the two builds of the same header differ in the order of the sums alone: the coarse curves agree to rounding, lag by lag"""
    case = sc.group("sampling")[0]
    d, h = sc.DeviceSeedImu.run(case["p"], *case["pick"]), sc.HostSeedImu.run(case["p"], *case["pick"])
    assert d["status"] == h["status"] == 0 and d["count"] == h["count"]
    np.testing.assert_allclose(d["coarse_J"], h["coarse_J"], rtol=1e-9)
    assert abs(d["time_offset"] - h["time_offset"]) < 1e-9


def test_refusals_that_need_a_device():
    import test_seed_imu_cpu as cpu
    assert cpu.sweep_rc() == 0 and cpu.seed_rc() == 0
    assert cpu.sweep_rc(device=4096) == NO_DEVICE and cpu.seed_rc(device=4096) == NO_DEVICE
    assert cpu.sweep_rc(device=4096, n_lags=0) == BAD_ARG                      # (the arguments are judged first)
    p = cpu._small()
    t = lib.time_seed_imu(*sc.DeviceSeedImu._args(p), np.linspace(-0.1, 0.1, 41), reps=2)
    assert t["prepare"] > 0.0 and t["sweep"] > 0.0 and t["gravity"] > 0.0
    # every lag outside the log: status 1 from the library as from the reference, nothing else filled
    far = dict(p, imu_t=p["imu_t"] + 100.0)
    r = lib.seed_imu(*sc.DeviceSeedImu._args(far))
    assert r["status"] == 1 and "time_offset" not in r and np.all(np.isinf(r["coarse_J"]))
    # an offset outside the range: the minimum on the edge, status 2
    late = sc.regular(100, offset=0.3, pad=0.6, seed=8)
    r = lib.seed_imu(*sc.DeviceSeedImu._args(late), range_s=0.1)
    assert r["status"] == 2 == ref.seed(late, 0.1, 0.0, 8)["status"]
    assert lib.seed_imu(*sc.DeviceSeedImu._args(late), range_s=0.5)["status"] == 0


# ------------------------------------------------------------------------------------------------ a calibration from the seed
@functools.lru_cache(maxsize=None)
def vi_problem(n_frames=60):
    """the generator's kb4 visual-inertial problem with the clocks 0.12 s apart; noise-free, as the problem of tests/test_vi_sim.py is, so
    that its tolerances apply"""
    return synth.generate(synth.Config(models=("kb4",), n_frames=n_frames, imu=True, seed=5, pixel_sigma=0.0, imu_noise=False, imu_truth=dict(time_offset=OFFSET)))


def camera_rotations(p, frame_time):
    """camera 0's rotation in the world at every frame from one batched planar PnP on its detections with the start intrinsics"""
    tiles = [t for t in p.tiles if t[1] == 0 and len(t[2]) >= 4]
    off = np.concatenate([[0], np.cumsum([len(t[2]) for t in tiles])]).astype(np.int32)
    pw = np.concatenate([p.grid_points[t[2]] for t in tiles]); pc = np.concatenate([t[3] for t in tiles])
    r = lib.pnp_planar_batch([p.cam_model[0]] * len(tiles), [p.cam_K_init[0]] * len(tiles), off, pw, pc)
    q = np.tile([0.0, 0.0, 0.0, 1.0], (len(frame_time), 1)); ok = np.zeros(len(frame_time), dtype=np.uint8)
    for v, t in enumerate(tiles):
        if r["status"][v] == 0:
            q[t[0]] = r["T_cw"][v, :4] * np.array([-1.0, -1.0, -1.0, 1.0]); ok[t[0]] = 1
    return q, ok


def rotation_to_quat(R):
    """as the command line prints it: [x y z w], w >= 0"""
    R = np.asarray(R).reshape(9)
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0); q = [(R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s, 0.25 * s]
    elif R[0] > R[4] and R[0] > R[8]:
        s = 2.0 * np.sqrt(1.0 + R[0] - R[4] - R[8]); q = [0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s, (R[7] - R[5]) / s]
    elif R[4] > R[8]:
        s = 2.0 * np.sqrt(1.0 + R[4] - R[0] - R[8]); q = [(R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s, (R[2] - R[6]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[8] - R[0] - R[4]); q = [(R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s, (R[3] - R[1]) / s]
    q = np.array(q)
    return q * ((-1.0 if q[3] < 0.0 else 1.0) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))


def _se3_log_norm(M):
    from scipy.spatial.transform import Rotation as R
    w = R.from_matrix(M[:3, :3]).as_rotvec()
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    k = 1.0 / 12.0 if th < 1e-10 else (1.0 - th / (2.0 * np.tan(th / 2.0))) / (th * th)
    return np.linalg.norm(np.concatenate([(np.eye(3) - 0.5 * W + k * (W @ W)) @ M[:3, 3], w]))


def _mat(T):
    from scipy.spatial.transform import Rotation as R
    M = np.eye(4); M[:3, :3] = R.from_quat(T[:4]).as_matrix(); M[:3, 3] = T[4:]
    return M


def calibration_errors(p, K, T_ck, rmse, ts, offset):
    return dict(logdiff=_se3_log_norm(_mat(p.cam_T_ck_gt[0]) @ np.linalg.inv(_mat(T_ck))), rmse=rmse, K=float(np.linalg.norm(K[:4] - p.cam_K_gt[0][:4])),
                offset=abs(ts - offset))


def assert_calibrated(e):
    assert e["logdiff"] < LOGDIFF_TOLERANCE and e["rmse"] < REPROJ_TOLERANCE and e["K"] < CAMERA_TOLERANCE and e["offset"] < TIMEOFFSET_TOLERANCE, e


def calibrate(p, seed):
    cal = lib.ViCalibrator(0)
    T_ck = p.cam_T_ck_init[0].copy()
    if seed is not None:
        T_ck[:4] = rotation_to_quat(seed["R_ck"])
    cal.AddCamera(p.cam_model[0], p.cam_K_init[0], T_ck, p.cfg.width, p.cfg.height)
    for n in range(len(p.frame_time)):
        cal.AddFrame(np.array([0, 0, 0, 1.0, 0, 0, 1000.0]), p.frame_time[n])
    for (f, c, ids, pix) in p.tiles:
        cal.AddObservations(f, c, p.grid_points[ids], pix)
    cal.AddImuMeasurements(p.imu_gyro, p.imu_accel, p.imu_t)
    if seed is not None:
        cal.SetTimeOffset(seed["time_offset"]); cal.SetGravity(seed["g_dir"]); cal.SetBiases(np.concatenate([seed["gyro_bias"], np.zeros(3)]))
    cal.SetPnPDevice(True)
    cal.InitFramePosesPnP()
    cal.SetOptimizationFlags(False, False, True, True)
    cal.SetMaxIters(100)
    cal.Solve()
    K, T = cal.GetCamera(0)
    return calibration_errors(p, K, T, cal.GetCameraProjRMSE()[0], cal.time_offset(), OFFSET), cal.trace(), cal.time_offset()


def test_a_calibration_from_the_seed_reaches_the_truth():
    p = vi_problem()
    q, ok = camera_rotations(p, p.frame_time)
    seed = lib.seed_imu(p.frame_time, q, ok, p.imu_t, p.imu_gyro, p.imu_accel)
    assert seed["status"] == 0 and ok.all()
    truth = dict(offset=OFFSET, R_ck=synth.quat_to_matrix(p.cam_T_ck_gt[0, :4]), bias=p.imu_gt["bg"], g_dir=p.imu_gt["g_dir"])
    print("seed:", sc.truth_errors(seed, truth), "rms / signal %.4f, %d intervals" % (seed["rms"] / seed["signal"], seed["count"]))
    e, trace, ts = calibrate(p, seed)
    print("seeded: %d trace rows, final offset %.6f s, errors %s" % (len(trace), ts, e))
    e0, trace0, ts0 = calibrate(p, None)                         # today's start, recorded, nothing asserted
    print("unseeded: %d trace rows, final offset %.6f s, errors %s" % (len(trace0), ts0, e0))
    assert_calibrated(e)


# ------------------------------------------------------------------------------------------------ the command line
def _run(args, cwd):
    return subprocess.run([BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _read_xml(path):
    s = open(path).read()
    block = s.split("<camera>")[1]
    params = [float(x) for x in re.search(r"<params>\s*\[(.*?)\]", block, re.S).group(1).split(";")]
    T = [float(x) for x in re.split(r"[,;]", re.search(r"<T_wc>\s*\[(.*?)\]", block, re.S).group(1))]
    return np.array(params), np.array(T).reshape(3, 4)


def test_cli_seed_imu(tmp_path):
    p = vi_problem()
    files, imu_dir = synth.write_dataset(p, str(tmp_path))
    out = tmp_path / "cameras.xml"
    r = _run(["-cam", "detections://" + files[0], "-imu", "csv://" + imu_dir, "-models", "kb4", "-max_iters", "100", "-seed_imu", "-nouse_system_time", "-output", str(out)],
             str(tmp_path))
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    # without system time the tool shifts the frames so that both streams begin together (today's start of the offset); the seed is relative to
    # the times the calibrator gets
    shift = p.imu_t[0] - p.frame_time[0]
    q, ok = camera_rotations(p, p.frame_time)
    seed = lib.seed_imu(p.frame_time + shift, q, ok, p.imu_t, p.imu_gyro, p.imu_accel)
    assert seed["status"] == 0
    m = re.search(r"^I -seed_imu: time offset (\S+) ms, R_ck \[qx qy qz qw\] (\S+) (\S+) (\S+) (\S+) \((\S+) degrees from identity\), gyro bias (\S+) (\S+) (\S+), "
                  r"gravity (\S+) (\S+), rms / signal (\S+), (\d+) intervals", r.stderr, re.M)
    assert m, r.stderr
    qs = rotation_to_quat(seed["R_ck"])
    assert m.group(1) == "%.6f" % (1e3 * seed["time_offset"]) and [m.group(k) for k in (2, 3, 4, 5)] == ["%.9f" % x for x in qs], (m.groups(), seed)
    angle = np.rad2deg(2.0 * np.arctan2(np.linalg.norm(qs[:3]), abs(qs[3])))
    assert int(m.group(13)) == seed["count"] and m.group(6) == "%.3f" % angle and m.group(12) == "%.4f" % (seed["rms"] / seed["signal"])
    assert [m.group(k) for k in (7, 8, 9, 10, 11)] == ["%.6g" % x for x in list(seed["gyro_bias"]) + list(seed["g_dir"])]
    assert "W -seed_imu" not in r.stderr
    params, T_wc = _read_xml(str(out))
    from scipy.spatial.transform import Rotation as R
    R_ck = (T_wc[:, :3] @ synth.RDF_ROBOTICS).T                               # T_wc = T_ck^-1 * SE3(RdfRobotics^-1, 0), as tests/test_cli.py reads it
    T_ck = np.concatenate([R.from_matrix(R_ck).as_quat(), -R_ck @ T_wc[:, 3]])
    ts = float(re.search(r"time offset: ([-0-9.e+]+) s", r.stdout).group(1))
    rmse = float(re.search(r"reprojection RMSE: ([-0-9.e+]+) px", r.stdout).group(1))
    e = calibration_errors(p, params, T_ck, rmse, ts, OFFSET + shift)
    print("command line:", e)
    assert_calibrated(e)


def test_cli_flag_conflicts_exit_1(tmp_path):
    data = str(tmp_path / "no_such_data")
    for extra in ([], ["-imu", "csv://" + data, "-nocalibrate_imu"], ["-imu", "csv://" + data, "-has_initial_guess"]):
        r = _run(["-cam", "detections://" + data + ".csv", "-models", "kb4", "-seed_imu"] + extra, str(tmp_path))
        assert r.returncode == 1 and r.stderr.startswith("ERROR:") and "seed_imu" in r.stderr, (extra, r.stdout + r.stderr)


def test_cli_declines_a_short_log_and_starts_as_without_the_flag(tmp_path):
    p = synth.generate(synth.Config(models=("kb4",), n_frames=20, imu=True, seed=5))
    files, imu_dir = synth.write_dataset(p, str(tmp_path))
    base = ["-cam", "detections://" + files[0], "-imu", "csv://" + imu_dir, "-models", "kb4", "-max_iters", "100"]
    a = _run(base + ["-output", str(tmp_path / "a.xml"), "-seed_imu", "-seed_imu_min_intervals", "30"], str(tmp_path))
    b = _run(base + ["-output", str(tmp_path / "b.xml")], str(tmp_path))
    assert a.returncode == b.returncode, a.stdout + a.stderr + b.stdout + b.stderr
    w = [l for l in a.stderr.splitlines() if l.startswith("W -seed_imu")]
    assert len(w) == 1 and "too few frame intervals" in w[0] and "I -seed_imu" not in a.stderr, a.stderr
    strip = lambda s: re.sub(r"solve time: \S+ s", "solve time", s).replace("a.xml", "b.xml")
    assert strip(a.stdout) == strip(b.stdout)
    assert open(tmp_path / "a.xml").read() == open(tmp_path / "b.xml").read()
