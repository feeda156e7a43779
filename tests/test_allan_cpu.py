"""The IMU noise characterisation (vc_allan*), the part that needs no GPU: its arithmetic (vc_allan.hpp) compiled for the host and run in plain
loops (tests/host_harness/allan_harness.cpp), held to the numpy reference (tests/allan_ref.py) by the checks of tests/allan_cases.py, the same
checks tests/test_allan_gpu.py applies to the kernels; the host-only entry points of the library (the factors, the fit); what the sigmas mean
to the solve's weights; the entry points' argument errors and their refusal to run without a device; the Python face's refusals; the
command line's flags.

Measured (host build): bound 7.2e-12 from the spreads edges 2.0e-16, sizes 7.2e-14, noise 1.9e-14, range 1.5e-15; worst adev error over the
bound: edges 1.1e-4, sizes 1.0e-2, noise 2.3e-3, range 6.8e-4.  The fit: bound 1.7e-10, worst over the bound 4.9e-3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import allan_cases as ac
import allan_ref as ref
import vicalib_amd.lib as lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG, NO_DEVICE, UNSUPPORTED = -2, -1, -7


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_cases_cover_what_they_claim():
    b, spreads, worst = ac.bound()          # (asserts the sizes against the header's constants and the reference against the truth)
    assert set(spreads) == set(ac.GROUPS) and 0.0 < b <= 1e-6
    assert worst["curve"] <= 4.0 and worst["N"] <= 0.02 and worst["K"] <= 0.15
    c = ac.constants()
    assert c["max_n"] == 1 << 24 and c["scan_block"] % 64 == 0 and c["chunk"] % 256 == 0
    assert len(ac.group("noise")) == 3 and all(len(l["time"]) == 65536 for l in ac.group("noise"))
    assert 0.0 < ac.fit_bound()[0] <= 1e-6
    ac.static_log()


@pytest.mark.parametrize("name", ac.GROUPS)
def test_host_build_matches_the_reference(name):
    ac.check(name, ac.run_group(name, ac.HostAllan), label=" (host build)")


def test_host_build_known_answers():
    ac.check_known(ac.HostAllan, " (host build)")


def test_host_build_channels_and_static_stretch():
    ac.check_channels(ac.HostAllan)
    ac.check_static(ac.HostAllan)


def test_fit_host_build_and_library():
    ac.check_fit(ac.host_fit, " (host build)")
    ac.check_fit(lib.allan_fit, " (library)")
    tau, av, e = ac.fit_cases()[1]
    assert lib.allan_fit(tau, av, e) == ac.host_fit(tau, av, e)


@pytest.mark.parametrize("n_used, per_decade, fraction", [(2, 20, 1.0 / 9.0), (9, 20, 1.0 / 9.0), (17, 20, 1.0 / 9.0), (18, 20, 1.0 / 9.0), (65536, 10, 1.0 / 9.0),
                                                          (1 << 21, 20, 1.0 / 9.0), (1 << 24, 20, 0.5), (4097, 3, 0.25), (1000, 1000, 0.5)])
def test_factors(n_used, per_decade, fraction):
    want = ref.factors(n_used, per_decade, fraction)
    for m, e in (ac.host_factors(n_used, per_decade, fraction), lib.allan_factors(n_used, per_decade, fraction)):
        assert m.tolist() == want.tolist()
        assert m[0] == 1 and np.all(np.diff(m) > 0) and 2 * int(m[-1]) <= n_used and m[-1] <= max(1, int(np.floor(n_used * fraction)))
        np.testing.assert_allclose(e, ref.rel_err(n_used, want), rtol=1e-15)
    if (n_used, per_decade) == (1 << 21, 20):
        assert len(want) == 97 and abs(ref.rel_err(9000, 1000) - 0.25) < 1e-15              # the issue's figures: 97 times at 2^21; 25 % at 1/9


def test_factors_refusals():
    L = lib.load()
    n_m = C.c_int(0)
    m = np.zeros(8, dtype=np.int32)
    call = lambda n, pd, fr, cap, mp, cnt=C.byref(n_m): L.vc_allan_factors(n, pd, C.c_double(fr), cap, mp, None, cnt)
    assert call(1000, 20, 1.0 / 9.0, 0, None) == 0 and n_m.value == len(ref.factors(1000, 20, 1.0 / 9.0))
    assert call(1, 20, 0.1, 0, None) == BAD_ARG and call(1000, 0, 0.1, 0, None) == BAD_ARG
    for fr in (0.0, -0.1, 0.51, float("nan")):
        assert call(1000, 20, fr, 0, None) == BAD_ARG, fr
    assert call(1000, 20, 0.1, 0, None, None) == BAD_ARG
    assert call(1000, 20, 1.0 / 9.0, 8, ac._p(m)) == BAD_ARG                                 # more factors than the caller has room for
    assert call(20, 20, 1.0 / 9.0, 8, ac._p(m)) == 0 and m[:n_m.value].tolist() == [1, 2]
    out = np.zeros(5); mask = C.c_int(0)
    t = np.ones(4)
    assert L.vc_allan_fit(0, ac._p(t), ac._p(t), ac._p(t), ac._p(out), C.byref(mask)) == BAD_ARG
    assert L.vc_allan_fit(4, None, ac._p(t), ac._p(t), ac._p(out), C.byref(mask)) == BAD_ARG
    assert L.vc_allan_fit(4, ac._p(t), ac._p(t), ac._p(t), None, C.byref(mask)) == BAD_ARG
    assert L.vc_allan_fit(4, ac._p(t), ac._p(t), ac._p(t), ac._p(out), None) == BAD_ARG


def test_sigma_is_the_per_sample_deviation_the_weights_expect():
    """a block of T seconds at step dt with gyro noise alone, through the maps and the noise term of the solve's weights: the rotation
    variance at the block's end is sigma^2 dt T, and it halves with the step.  So the solve's sigma is a per-sample standard deviation at the
    log's rate, and a white-noise density N gives sigma = N / sqrt(tau0)."""
    out = np.zeros(3)
    sigma, dt, T = 5.3088444e-5, 0.005, 0.5
    ac.harness().allan_harness_gyro_variance(C.c_double(sigma), C.c_double(dt), C.c_double(T), ac._p(out))
    assert abs(out[0] / (sigma * sigma * dt * T) - 1.0) < 1e-9 and out[1] == sigma * sigma * dt * T
    assert abs(out[2] / out[0] - 0.5) < 1e-9
    N = sigma * np.sqrt(dt)                        # the density that gives the same angle random walk at any rate: variance N^2 T
    assert abs(out[0] / (N * N * T) - 1.0) < 1e-9


# ---------------------------------------------------------------------------------------------- refusals
def _create(n=64, gyro=True, accel=True, time=True, out=True, device=0, edit=None):
    L = lib.load()
    log = ac._noise_log(max(n, 2) if n <= 1 << 20 else 8, 3)
    a = dict(gyro=log["gyro"].copy(), accel=log["accel"].copy(), time=log["time"].copy())
    if edit:
        edit(a)
    h = C.c_void_p()
    rc = L.vc_allan_create(device, n, ac._p(a["gyro"]) if gyro else None, ac._p(a["accel"]) if accel else None, ac._p(a["time"]) if time else None,
                           C.byref(h) if out else None)
    assert rc != 0 or h.value
    if h.value:
        L.vc_allan_destroy(h)
    return rc


def test_argument_errors_come_before_the_device():
    for missing in ("gyro", "accel", "time", "out"):
        assert _create(**{missing: False}) == BAD_ARG, missing
    assert _create(n=1) == BAD_ARG and _create(n=0) == BAD_ARG and _create(n=-5) == BAD_ARG
    assert _create(n=(1 << 24) + 1) == UNSUPPORTED                      # (eight samples behind the pointers: refused before they are read)
    assert _create(n=(1 << 24) + 1, device=-1) == UNSUPPORTED

    def set_at(key, idx, value):
        def edit(a):
            a[key][idx] = value
        return edit
    for bad in (np.nan, np.inf, -np.inf):
        assert _create(edit=set_at("time", 0, bad)) == BAD_ARG and _create(edit=set_at("time", 63, bad)) == BAD_ARG
        assert _create(edit=set_at("gyro", (17, 1), bad)) == BAD_ARG and _create(edit=set_at("accel", (63, 2), bad)) == BAD_ARG
    assert _create(edit=set_at("time", 10, 100.0 + 0.005 * 9)) == BAD_ARG               # equal to its predecessor
    assert _create(edit=set_at("time", 10, 99.0)) == BAD_ARG                            # decreasing
    assert _create(device=-1, edit=set_at("time", 10, 99.0)) == BAD_ARG                 # (the arguments are judged before the device)
    L = lib.load()
    m = np.array([1], dtype=np.int32); av = np.zeros(6)
    assert L.vc_allan_run(None, 1, ac._p(m), ac._p(av), None) == BAD_ARG and L.vc_allan_set_range(None, 0, 2) == BAD_ARG
    assert L.vc_allan_static(None, 1, C.c_double(0), C.c_double(0), None, None) == BAD_ARG and L.vc_allan_get(None, *([None] * 7)) == BAD_ARG
    assert L.vc_time_allan(None, 1, ac._p(m), 3, ac._p(av)) == BAD_ARG
    L.vc_allan_destroy(None)
    if not _have_gpu():          # no host fallback: a valid log without a device is refused
        assert _create() == NO_DEVICE and _create(n=2) == NO_DEVICE


def test_python_face_refuses_what_the_library_refuses():
    log = ac._noise_log(64, 3)
    with pytest.raises(lib.VicalibError):
        lib.AllanAnalyzer(log["gyro"][:, :2], log["accel"], log["time"])             # not n x 3
    with pytest.raises(lib.VicalibError):
        lib.AllanAnalyzer(log["gyro"], log["accel"][:-1], log["time"])               # lengths disagree
    with pytest.raises(lib.VicalibError):
        lib.AllanAnalyzer(log["gyro"], log["accel"], log["time"][:-1])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.AllanAnalyzer(log["gyro"][:1], log["accel"][:1], log["time"][:1])
    t = log["time"].copy(); t[5] = t[4]
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.AllanAnalyzer(log["gyro"], log["accel"], t)
    g = log["gyro"].copy(); g[3, 0] = np.nan
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.AllanAnalyzer(g, log["accel"], log["time"])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        lib.allan_factors(1000, 20, 0.75)
    with pytest.raises(lib.VicalibError):
        lib.allan_fit(np.ones(4), np.ones(3), np.ones(4))
    if not _have_gpu():
        with pytest.raises(lib.VicalibError, match="NO_DEVICE"):
            lib.AllanAnalyzer(log["gyro"], log["accel"], log["time"])


# ---------------------------------------------------------------------------------------------- the command line
def test_help_lists_the_flags():
    r = subprocess.run([BIN, "-help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    for flag in ("-allan_imu", "-allan_dir", "-allan_per_decade", "-allan_max_fraction", "-allan_static_window_s", "-allan_static_gyro", "-allan_static_accel",
                 "-static_accel_threshold", "-static_gyro_threshold"):
        assert flag in text, flag
    assert 'default: "5.3088444e-5"' in text and 'default: "0.001883649"' in text           # the defaults of -gyro_sigma / -accel_sigma stay


def test_flag_errors_exit_1_before_anything_else(tmp_path):
    """exit status 1 and the flag's name, with or without a GPU, before the log is opened (it does not exist) and nothing written"""
    log = "csv://" + str(tmp_path / "no_such_log")
    out = tmp_path / "allan"
    cases = [([], "-allan_dir"), (["-allan_dir", str(out), "-allan_per_decade", "0"], "allan_per_decade"),
             (["-allan_dir", str(out), "-allan_per_decade", "1001"], "allan_per_decade"), (["-allan_dir", str(out), "-allan_max_fraction", "0"], "allan_max_fraction"),
             (["-allan_dir", str(out), "-allan_max_fraction", "0.6"], "allan_max_fraction"), (["-allan_dir", str(out), "-allan_static_window_s", "0"], "allan_static_window_s"),
             (["-allan_dir", str(out), "-allan_static_window_s", "-2"], "allan_static_window_s"), (["-allan_dir", str(out), "-allan_static_gyro", "nan"], "allan_static_gyro")]
    for extra, word in cases:
        r = subprocess.run([BIN, "-allan_imu", log] + extra, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 1 and r.stderr.startswith("ERROR:") and word in r.stderr, (extra, r.stdout + r.stderr)
        assert not out.exists()
    r = subprocess.run([BIN, "-allan_dir", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "-allan_imu" in r.stderr and not out.exists()
    # a log that cannot be read is an error of its own, after the flags: exit 1, no device needed to say so
    r = subprocess.run([BIN, "-allan_imu", log, "-allan_dir", str(out)], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "cannot open" in r.stderr and not out.exists()


def test_cli_without_a_device_exits_3(tmp_path):
    if _have_gpu():
        return          # (with a device the same command line is tests/test_allan_gpu.py's)
    log = ac._noise_log(400, 9)
    d = tmp_path / "log"
    d.mkdir()
    np.savetxt(d / "gyro.txt", log["gyro"]); np.savetxt(d / "accel.txt", log["accel"]); np.savetxt(d / "timestamp.txt", log["time"], fmt="%.9f")
    r = subprocess.run([BIN, "-allan_imu", "csv://" + str(d), "-allan_dir", str(tmp_path / "allan")], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 3 and "no HIP device" in r.stderr, r.stdout + r.stderr
