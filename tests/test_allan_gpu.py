"""The IMU noise characterisation on the device (vc_allan*: block totals, a scan of the totals, blocks that scan with their carry; a sweep over
(chunk, factor, channel) with one partial each and a finishing kernel; one byte per window start) against the numpy reference
(tests/allan_ref.py), on the logs of tests/allan_cases.py with that file's checks: adev of every point within 100 times the spread between the
reference's float64 and longdouble routes, term counts and the static stretch's integers exactly, the known answers, bytes for a channel
alone and for a second run.  The refusals that need a handle.  Then the command line's -allan_imu.

Measured (MI355X): see DESIGN 4.18."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import allan_cases as ac
import allan_ref as ref
import vicalib_amd.lib as lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
BAD_ARG = -2


@pytest.mark.parametrize("name", ac.GROUPS)
def test_device_matches_the_reference(name):
    ac.check(name, ac.run_group(name, lib.AllanAnalyzer), label=" (device)")


def test_known_answers():
    ac.check_known(lib.AllanAnalyzer, " (device)")


def test_a_channel_gives_the_same_bits_alone_and_again():
    ac.check_channels(lib.AllanAnalyzer)


def test_static_stretch():
    ac.check_static(lib.AllanAnalyzer)


def test_what_the_handle_reports():
    log = ac.group("range")[0]
    t = log["time"].copy()
    t[1000:] += 0.004                      # one interval of 1.8 tau0
    t[2000:] += 0.0101                     # and one of 3 tau0
    a = lib.AllanAnalyzer(log["gyro"], log["accel"], t)
    g = a.get()
    tau0, lo, hi, irr = ref.log_info(t)
    assert g["n"] == 3000 and g["range"] == (0, 3000) and g["irregular"] == irr == 2
    assert g["tau0"] == tau0 and g["dt_min"] == lo and g["dt_max"] == hi
    np.testing.assert_allclose(g["means"], ref.channels(log["gyro"], log["accel"]).mean(axis=1), rtol=1e-13)
    # the same handle before and after set_range, and back: the first run's bytes again
    m = np.array([1, 2, 7, 100], dtype=np.int32)
    whole, terms = a.run(m)
    a.set_range(517, 1301)
    assert a.get()["range"] == (517, 1301)
    part, part_terms = a.run(m)
    assert part_terms.tolist() == [1301 - 2 * int(x) + 1 for x in m] and terms.tolist() == [3000 - 2 * int(x) + 1 for x in m]
    assert ac._rel(part, ref.avar6(log["gyro"], log["accel"], m, 517, 1301, np.longdouble)) <= ac.bound()[0]
    a.set_range(0, 3000)
    assert a.run(m)[0].tobytes() == whole.tobytes()
    assert a.time(m, reps=2)["sweep"] > 0.0
    assert a.run(m)[0].tobytes() == whole.tobytes()                      # (the timer wrote the same sums again)
    a.close()


def test_refusals_that_need_a_handle():
    log = ac._noise_log(64, 3)
    a = lib.AllanAnalyzer(log["gyro"], log["accel"], log["time"])
    L = lib.load()
    av = np.zeros(12)

    def run(m, out=True, n_m=None):
        m = np.array(m, dtype=np.int32)
        return L.vc_allan_run(a.h, len(m) if n_m is None else n_m, ac._p(m), ac._p(av) if out else None, None)
    assert run([1, 32]) == 0
    assert run([0]) == BAD_ARG and run([-3]) == BAD_ARG and run([1, 33]) == BAD_ARG and run([1], out=False) == BAD_ARG and run([1], n_m=0) == BAD_ARG
    assert L.vc_allan_run(a.h, 1, None, ac._p(av), None) == BAD_ARG
    for first, count in ((-1, 10), (0, 1), (0, 65), (60, 5), (64, 2), (0, 0), (1, 2 ** 31 - 1)):
        assert L.vc_allan_set_range(a.h, first, count) == BAD_ARG, (first, count)
    assert a.get()["range"] == (0, 64)
    assert L.vc_allan_set_range(a.h, 62, 2) == 0 and run([1]) == 0 and run([2]) == BAD_ARG                 # a factor is judged against the range in use
    assert L.vc_allan_set_range(a.h, 0, 64) == 0
    static = lambda w, g=1.0, ac_=1.0: L.vc_allan_static(a.h, w, C.c_double(g), C.c_double(ac_), None, None)
    assert static(0) == BAD_ARG and static(-1) == BAD_ARG and static(32) == BAD_ARG and static(2 ** 30) == BAD_ARG
    assert static(31) in (0, 1) and static(3, float("nan")) == BAD_ARG and static(3, 1.0, float("nan")) == BAD_ARG
    assert L.vc_time_allan(a.h, 1, ac._p(np.array([1], dtype=np.int32)), 0, ac._p(av)) == BAD_ARG
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        a.run([40])
    with pytest.raises(lib.VicalibError):
        a.run([])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        a.set_range(10, 60)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        a.static(40, 1.0, 1.0)
    a.close()


# ------------------------------------------------------------------------------------------------ the command line
def _write_log(d, log):
    d.mkdir()
    np.savetxt(d / "gyro.txt", log["gyro"], fmt="%.17g"); np.savetxt(d / "accel.txt", log["accel"], fmt="%.17g"); np.savetxt(d / "timestamp.txt", log["time"], fmt="%.17g")


def test_cli_allan(tmp_path):
    """a generated static log of 16 384 samples: allan.csv agrees with a library run on the same arrays to the printed digits, the summary
    holds the sigmas N / sqrt(tau0), the pasted line parses and holds the quadratic means"""
    n = 16384
    log = ac._noise_log(n, 21)
    _write_log(tmp_path / "log", log)
    out = tmp_path / "allan"
    r = subprocess.run([BIN, "-allan_imu", "csv://" + str(tmp_path / "log"), "-allan_dir", str(out), "-allan_per_decade", "10"], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    a = lib.AllanAnalyzer(log["gyro"], log["accel"], log["time"])
    tau0 = a.get()["tau0"]
    m, e = lib.allan_factors(n, 10, 1.0 / 9.0)
    avar, terms = a.run(m)
    a.close()
    fits = [lib.allan_fit(tau0 * m, avar[c], e) for c in range(6)]
    lines = open(out / "allan.csv").read().splitlines()
    assert lines[0] == "tau,m,terms,rel_err," + ",".join("adev_" + c for c in ref.CHANNELS) + "," + ",".join("model_" + c for c in ref.CHANNELS)
    assert len(lines) == len(m) + 1
    for j, line in enumerate(lines[1:]):
        want = ["%.10e" % (tau0 * m[j]), "%d" % m[j], "%d" % terms[j], "%.10e" % e[j]] + ["%.10e" % np.sqrt(avar[c, j]) for c in range(6)]
        want += ["%.10e" % np.sqrt(ref.model(f["N"], f["B"], f["K"], tau0 * m[j:j + 1])[0]) for f in fits]
        got = line.split(",")
        assert got[:10] == want[:10], (j, got, want)
        np.testing.assert_allclose([float(x) for x in got[10:]], [float(x) for x in want[10:]], rtol=1e-9)      # (the model: libm against numpy)
    rows = [l.split(",") for l in open(out / "allan_summary.csv").read().splitlines()]
    assert rows[0][:4] == ["axis", "mean", "adev_tau0", "N"] and [r_[0] for r_ in rows[1:]] == list(ref.CHANNELS)
    col = {k: i for i, k in enumerate(rows[0])}
    sig = []
    for c, row in enumerate(rows[1:]):
        assert int(row[col["fit_status"]]) == 0 and "N" in row[col["active_terms"]]
        assert row[col["N"]] == "%.10e" % fits[c]["N"] and row[col["sigma"]] == "%.10e" % (fits[c]["N"] / np.sqrt(tau0))
        assert row[col["adev_tau0"]] == "%.10e" % np.sqrt(avar[c, 0]) and (int(row[col["n"]]), int(row[col["first"]]), int(row[col["count"]])) == (n, 0, n)
        assert int(row[col["irregular_intervals"]]) == 0
        sig.append(fits[c]["N"] / np.sqrt(tau0))
    # white noise of a known sigma: the per-sample sigma comes back within 3 % on every axis
    truth = np.concatenate([ac.SIGMA * np.array([1.0, 0.7, 1.6]), 10 * ac.SIGMA * np.array([0.9, 1.3, 1.0])])
    np.testing.assert_allclose(sig, truth, rtol=0.03)
    p = re.search(r"^-gyro_sigma (\S+) -accel_sigma (\S+)$", r.stdout, re.M)
    assert p, r.stdout
    np.testing.assert_allclose([float(p.group(1)), float(p.group(2))], [np.sqrt(np.mean(np.square(sig[:3]))), np.sqrt(np.mean(np.square(sig[3:])))], rtol=1e-7)
    assert len(re.findall(r"^I (gyro|accel) white noise N = ", r.stderr, re.M)) == 2
    assert "W the range used is 81.9 s long" in r.stderr and "intervals lie outside" not in r.stderr and "failed" not in r.stderr


def test_cli_allan_static_stretch_and_warnings(tmp_path):
    """the log of the static group, with a dropout: the stretch found is the library's, the irregular intervals are reported, not refused"""
    log = ac.static_log()
    t = log["time"].copy()
    for k in range(100, 6000, 60):
        t[k:] += 0.01                          # 99 intervals of 3 tau0: 1.65 % of the log
    _write_log(tmp_path / "log", dict(log, time=t))
    out = tmp_path / "allan"
    tau0 = ref.log_info(t)[0]
    r = subprocess.run([BIN, "-allan_imu", "csv://" + str(tmp_path / "log"), "-allan_dir", str(out), "-allan_static_window_s", "%.6f" % (ac.STATIC_W * tau0),
                        "-allan_static_gyro", str(ac.STATIC_THR[0]), "-allan_static_accel", str(ac.STATIC_THR[1])], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ref.static(log["gyro"], log["accel"], ac.STATIC_W, *ac.STATIC_THR)
    rows = [l.split(",") for l in open(out / "allan_summary.csv").read().splitlines()]
    col = {k: i for i, k in enumerate(rows[0])}
    assert (int(rows[1][col["first"]]), int(rows[1][col["count"]])) == (want[1], want[2]) and int(rows[1][col["irregular_intervals"]]) == 99
    assert "W 99 of 5999 intervals lie outside" in r.stderr and re.search(r"^I static stretch: samples %d \.\.\. %d of 6000" % (want[1], want[1] + want[2] - 1), r.stderr, re.M)
    # thresholds nothing passes: an error of its own, exit 1, no files
    out2 = tmp_path / "allan2"
    r = subprocess.run([BIN, "-allan_imu", "csv://" + str(tmp_path / "log"), "-allan_dir", str(out2), "-allan_static_gyro", "1e-9"], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path))
    assert r.returncode == 1 and "quiet" in r.stderr and not (out2 / "allan.csv").exists(), r.stdout + r.stderr
