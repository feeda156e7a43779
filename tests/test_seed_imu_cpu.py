"""The inertial seed (vc_seed_imu*), the part that needs no GPU: its arithmetic (vc_seed_imu.hpp) compiled for the host and run in plain loops
(tests/host_harness/seed_imu_harness.cpp), held to the numpy reference (tests/seed_imu_ref.py) by the checks of tests/seed_imu_cases.py, the
same checks tests/test_seed_imu_gpu.py applies to the kernels; the entry points' argument errors and their refusal to run without a device;
the Python face's refusals; the command line's flags.

Measured (host build): bound 1.4e-9 from the spreads edges 1.4e-11, sizes 2.3e-12, sampling 9.5e-13, truth 1.2e-12; worst error over the
bound: edges 4.6e-2, sizes 3.6e-3, sampling 3.3e-2, truth 3.0e-2.  The reference against the truth (200 frames at 0.003, 0.12, -0.2 s and 60
frames at 0.12 s, rotations at 0.1 degrees): offset 0.76 ms, rotation 0.45 degrees, gyro bias 1.04e-3 rad/s, gravity angles 5.8e-3 rad; the
limits are three times those, rounded up.  20 frames at 0.12 s, the documented failure: offset 17.8 ms, rotation 18.0 degrees off,
rms / signal 0.48."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_imu_cases as sc
import seed_imu_ref as ref
import vicalib_amd.lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE, UNSUPPORTED = -2, -1, -7


def _have_gpu():
    """(the device node first: where it exists torch is not asked -- a second HIP runtime initialised in this process after the library's
    has been seen to report no device on a machine that has one)"""
    if os.path.exists("/dev/kfd"):
        return True
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_cases_cover_what_they_claim():
    b, spreads, worst = sc.bound()          # (asserts the sizes against the header's constants and the reference against the truth)
    assert set(spreads) == set(sc.GROUPS) and 0.0 < b <= 1e-6
    assert all(worst[k] <= sc.TRUTH_LIMITS[k] <= 3.5 * worst[k] for k in worst), worst
    sc.known_cases()
    # the documented failure: one second of motion does not determine the seed; recorded, not asserted
    p = sc.synth_problem(*sc.FAIL_CASE)
    r = ref.seed(p, 0.5, 0.0, 8)
    if r["status"] == 0:
        print("20 frames:", sc.truth_errors(r, p["truth"]), "rms / signal %.3f" % (r["rms"] / r["signal"]))


@pytest.mark.parametrize("name", sc.GROUPS)
def test_host_build_matches_the_reference(name):
    sc.check(name, sc.HostSeedImu, label=" (host build)")


def test_host_build_known_answers():
    sc.check_known(sc.HostSeedImu, " (host build)")


def test_host_build_bytes():
    sc.check_bytes(sc.HostSeedImu)


# ---------------------------------------------------------------------------------------------- refusals
def _small():
    return sc.regular(12, seed=3)


def sweep_rc(p=None, device=0, n_lags=1, lags=True, edit=None, null=(), n_frames=None, n_samples=None):
    """the status of vc_seed_imu_sweep on a small problem with one thing wrong"""
    L = lib.load()
    p = dict(p or _small())
    a = {k: np.array(p[k], dtype=np.uint8 if k == "frame_ok" else np.float64) for k in ("frame_t", "frame_q", "frame_ok", "imu_t", "gyro", "accel")}
    a["lags"] = np.zeros(max(n_lags, 1))
    a["max_gap_s"], a["min_intervals"] = p["max_gap_s"], p["min_intervals"]
    if edit:
        edit(a)
    ptr = lambda k: None if k in null or (k == "lags" and not lags) else sc._p(a[k])
    J = np.zeros(max(n_lags, 1))
    return L.vc_seed_imu_sweep(device, len(a["frame_t"]) if n_frames is None else n_frames, ptr("frame_t"), ptr("frame_q"), ptr("frame_ok"),
                               len(a["imu_t"]) if n_samples is None else n_samples, ptr("imu_t"), ptr("gyro"), ptr("accel"), C.c_double(a["max_gap_s"]),
                               int(a["min_intervals"]), n_lags, ptr("lags"), sc._p(J), None, None, None, None)


def seed_rc(device=0, range_s=0.2, step_s=0.0, fine=4, status=True, null=(), p=None):
    L = lib.load()
    p = p or _small()
    a = {k: np.array(p[k], dtype=np.uint8 if k == "frame_ok" else np.float64) for k in ("frame_t", "frame_q", "frame_ok", "imu_t", "gyro", "accel")}
    ptr = lambda k: None if k in null else sc._p(a[k])
    st = C.c_int(-1)
    return L.vc_seed_imu(device, len(a["frame_t"]), ptr("frame_t"), ptr("frame_q"), ptr("frame_ok"), len(a["imu_t"]), ptr("imu_t"), ptr("gyro"), ptr("accel"),
                         C.c_double(p["max_gap_s"]), int(p["min_intervals"]), C.c_double(range_s), C.c_double(step_s), int(fine), None, None, None, None, None, None, None,
                         C.byref(st) if status else None, 0, None, None, None)


def _set(key, idx, value):
    def edit(a):
        a[key][idx] = value
    return edit


def test_argument_errors_come_before_the_device():
    for device in (0, -1):                                                   # (-1: no such device; the arguments are judged first)
        for missing in ("frame_t", "frame_q", "frame_ok", "imu_t", "gyro", "accel"):
            assert sweep_rc(device=device, null=(missing,)) == BAD_ARG, missing
            assert seed_rc(device=device, null=(missing,)) == BAD_ARG, missing
        assert sweep_rc(device=device, lags=False) == BAD_ARG and sweep_rc(device=device, n_lags=0) == BAD_ARG and sweep_rc(device=device, n_lags=-3) == BAD_ARG
        assert sweep_rc(device=device, n_frames=1) == BAD_ARG and sweep_rc(device=device, n_samples=1) == BAD_ARG and sweep_rc(device=device, n_frames=0) == BAD_ARG
        assert sweep_rc(device=device, n_samples=(1 << 24) + 1) == UNSUPPORTED          # (a small log behind the pointers: refused before it is read)
        for bad in (np.nan, np.inf, -np.inf):
            assert sweep_rc(device=device, edit=_set("frame_t", 0, bad)) == BAD_ARG and sweep_rc(device=device, edit=_set("frame_t", 12, bad)) == BAD_ARG
            assert sweep_rc(device=device, edit=_set("imu_t", 0, bad)) == BAD_ARG and sweep_rc(device=device, edit=_set("imu_t", 7, bad)) == BAD_ARG
            assert sweep_rc(device=device, edit=_set("gyro", (17, 1), bad)) == BAD_ARG and sweep_rc(device=device, edit=_set("accel", (0, 2), bad)) == BAD_ARG
            assert sweep_rc(device=device, edit=_set("lags", 0, bad)) == BAD_ARG
            assert seed_rc(device=device, range_s=bad) == BAD_ARG
        assert sweep_rc(device=device, edit=_set("frame_t", 5, 1.0 + 4 / 20.0)) == BAD_ARG          # equal to its predecessor
        assert sweep_rc(device=device, edit=_set("frame_t", 5, 0.5)) == BAD_ARG                     # decreasing
        assert sweep_rc(device=device, edit=_set("imu_t", 9, 0.0)) == BAD_ARG
        assert sweep_rc(device=device, edit=_set("frame_q", 3, [0.0, 0.0, 0.0, 0.49])) == BAD_ARG   # the norm of an ok frame's quaternion: [0.5, 2]
        assert sweep_rc(device=device, edit=_set("frame_q", 3, [0.0, 2.01, 0.0, 0.0])) == BAD_ARG
        assert sweep_rc(device=device, edit=_set("frame_q", 3, [np.nan, 0.0, 0.0, 1.0])) == BAD_ARG

        def key(k, v):
            def edit(a):
                a[k] = v
            return edit
        for gap in (0.0, -1.0, np.nan):
            assert sweep_rc(device=device, edit=key("max_gap_s", gap)) == BAD_ARG
        assert sweep_rc(device=device, edit=key("min_intervals", 0)) == BAD_ARG
        assert seed_rc(device=device, range_s=0.0) == BAD_ARG and seed_rc(device=device, range_s=-0.1) == BAD_ARG and seed_rc(device=device, fine=0) == BAD_ARG
        assert seed_rc(device=device, status=False) == BAD_ARG and seed_rc(device=device, range_s=1e9, step_s=1e-3) == BAD_ARG       # a lattice beyond 2^20 lags
    assert sweep_rc(device=-1) == NO_DEVICE and seed_rc(device=-1) == NO_DEVICE
    ms = np.zeros(3)
    p = _small()
    args = sc._arrays(p)
    call = lambda reps, out: lib.load().vc_time_seed_imu(0, len(args[0]), sc._p(args[0]), sc._p(args[1]), sc._p(args[2]), len(args[3]), sc._p(args[3]), sc._p(args[4]),
                                                         sc._p(args[5]), C.c_double(0.5), 10, 1, sc._p(np.zeros(1)), reps, out)
    assert call(0, sc._p(ms)) == BAD_ARG and call(3, None) == BAD_ARG
    if not _have_gpu():          # no host fallback: a valid problem without a device is refused
        assert sweep_rc() == NO_DEVICE and seed_rc() == NO_DEVICE and call(3, sc._p(ms)) == NO_DEVICE


def test_a_quaternion_of_a_frame_that_is_not_ok_is_not_judged():
    def edit(a):
        a["frame_q"][3] = 0.0
        a["frame_ok"][3] = 0
    assert sweep_rc(device=-1, edit=edit) == NO_DEVICE                       # (past the arguments)


def test_python_face_refuses_what_the_library_refuses():
    p = _small()
    a = sc.DeviceSeedImu._args(p)
    with pytest.raises(lib.VicalibError):
        lib.seed_imu_sweep(a[0], a[1][:, :3], *a[2:], [0.0])                 # not n x 4
    with pytest.raises(lib.VicalibError):
        lib.seed_imu(a[0], a[1], a[2][:-1], *a[3:])                          # lengths disagree
    with pytest.raises(lib.VicalibError):
        lib.seed_imu(*a[:4], a[4][:-1], a[5])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_imu_sweep(*a, [])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_imu(*a, range_s=0.0)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.seed_imu(a[0][:1], a[1][:1], a[2][:1], *a[3:])
    if not _have_gpu():
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.seed_imu(*a)
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.seed_imu_sweep(*a, [0.0])


# ---------------------------------------------------------------------------------------------- the command line
def test_help_lists_the_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("-seed_imu ", "-seed_imu_range", "-seed_imu_step", "-seed_imu_max_gap", "-seed_imu_min_intervals"):
        assert flag in text, flag


def test_flag_conflicts_exit_1_before_anything_is_read(tmp_path):
    """-seed_imu without -imu, with -nocalibrate_imu or with -has_initial_guess: exit status 1 and the flag's name, with or without a GPU,
    before the data set is opened (it does not exist)"""
    data = str(tmp_path / "no_such_data")
    for extra in ([], ["-imu", "csv://" + data, "-nocalibrate_imu"], ["-imu", "csv://" + data, "-has_initial_guess"]):
        r = subprocess.run([BIN, "-grid_preset", "small", "-cam", "file://" + data + "/*.pgm", "-seed_imu"] + extra, capture_output=True, text=True, timeout=60,
                           cwd=str(tmp_path))
        assert r.returncode == 1 and r.stderr.startswith("ERROR:") and "seed_imu" in r.stderr, (extra, r.stdout + r.stderr)
    for flag, value in (("-seed_imu_range", "0"), ("-seed_imu_max_gap", "-1"), ("-seed_imu_min_intervals", "0"), ("-seed_imu_step", "nan")):
        r = subprocess.run([BIN, "-grid_preset", "small", "-cam", "file://" + data + "/*.pgm", "-imu", "csv://" + data, "-seed_imu", flag, value], capture_output=True,
                           text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 1 and r.stderr.startswith("ERROR:") and flag[1:] in r.stderr, (flag, r.stdout + r.stderr)
