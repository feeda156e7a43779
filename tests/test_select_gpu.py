"""Greedy D-optimal view selection on the device (vc_selector*, vc_select.hip) through the C ABI: the cases and checks of tests/select_cases.py that
tests/test_select_cpu.py applies to the host build, the kernels against that host build, bitwise repeatability, a frame alone against the same frame
among 300, the calibrator's own selector against a standalone one, the run's argument errors and the command line end to end."""
import csv
import os
import re
import subprocess

import numpy as np
import pytest

import select_cases as sc
import select_ref as ref
import vicalib_amd.lib as lib
from vicalib_amd import synth
from vicalib_amd.lib import Selector, ViCalibrator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")


def selector_of(case):
    s = Selector(case["cameras"])
    tf, tc, off, pid = sc.flat(case)
    s.set_poses(case["poses"])
    s.add_tiles(tf, tc, off, case["points"], pid)
    return s


def read(s, with_information=True):
    out = dict(s.result())
    out.update(s.frames())
    out["last_gains"] = s.last_gains()
    if with_information:
        out["I"] = np.stack([s.frame_information(f)[0] for f in range(s.n_frames)])
        out["scale"] = s.frame_information(0)[1]
    return out


def device_select(case, k=None, start=None, prior=None, with_information=True):
    s = selector_of(case)
    s.run(case["k"] if k is None else k, case["start"] if start is None else start, case["prior"] if prior is None else prior)
    return read(s, with_information)


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = device_select(sc.cases()[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", sc.NAMES)
def test_information_matches_analytic_reference(runs, name):
    sc.check_information(name, runs(name))


@pytest.mark.parametrize("name", sc.NAMES)
def test_selection_follows_the_pick_rule(runs, name):
    got = runs(name)
    sc.check_selection(name, got)
    if sc.separation(name) >= sc.SEPARATION:
        assert np.array_equal(got["order"], sc.selection(name, True)["order"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_against_host_build(runs, name):
    """each of the two is within the case's tolerance of the reference, so they are within twice that of each other; the counts and, where the gains
    are well separated, the order are the same"""
    rc, host = sc.host_select(sc.cases()[name])
    assert rc == 0
    got, tol, a = runs(name), sc.tolerances(name), sc.analytic(name)
    for key in ("status", "corners", "behind"):
        assert np.array_equal(got[key], host[key])
    eI = float(np.abs(ref.scaled(got["I"] - host["I"], a["scale"])).max())
    es = float(np.abs(got["scale"] / host["scale"] - 1).max())
    print(f"{name}: device - host: I_f {eI:.3e} (tol {2 * tol['I']:.3e}), scale {es:.3e}")
    assert eI <= 2 * tol["I"] and es <= 2 * tol["scale"]
    assert len(got["order"]) == len(host["order"])
    if sc.separation(name) >= sc.SEPARATION:
        assert np.array_equal(got["order"], host["order"])
        assert np.abs(got["gain"] - host["gain"]).max() <= 2 * tol["gain"]
        assert np.abs(got["cum"] - host["cum"]).max() <= 2 * tol["cum"]
        left = host["last_gains"] >= 0
        assert np.array_equal(left, got["last_gains"] >= 0)
        assert np.abs(got["last_gains"] - host["last_gains"])[left].max(initial=0.0) <= 2 * tol["gain"]
    assert abs(got["total"] - host["total"]) <= 2 * tol["total"]


def test_unsupported_beyond_64_columns():
    with pytest.raises(lib.VicalibError, match="UNSUPPORTED"):
        Selector(sc.unsupported_case()["cameras"])


def test_two_runs_are_bitwise_equal(runs):
    for name in ("stereo_fov", "poly3_67", "rational6_x4"):
        again = device_select(sc.cases()[name])
        got = runs(name)
        for key in ("order", "gain", "cum", "I", "scale", "last_gains"):
            assert np.array_equal(again[key], got[key]), (name, key)
        assert again["total"] == got["total"]
    # ... and a second run on the same handle
    s = selector_of(sc.cases()["stereo_fov"])
    s.run(4)
    a = read(s)
    s.run(4)
    b = read(s)
    assert all(np.array_equal(a[k], b[k]) for k in ("order", "gain", "cum", "I", "last_gains")) and a["total"] == b["total"]


def test_a_frame_alone_and_among_300(runs):
    name = "fov_300"
    c, got = sc.cases()[name], runs(name)
    for f in (0, 1, 131, 299):                       # first and second wavefront of a workgroup, the middle, the last
        alone = dict(c, poses=c["poses"][f:f + 1], tiles=[(0, cam, ids) for (g, cam, ids) in c["tiles"] if g == f], k=1)
        one = device_select(alone)
        assert np.array_equal(one["I"][0], got["I"][f]), f
        assert one["status"][0] == got["status"][f] and one["corners"][0] == got["corners"][f]


def test_gains_never_grow():
    name = "stereo_fov"
    tol = sc.tolerances(name)["gain"]
    s = selector_of(sc.cases()[name])
    prev = None
    for k in (1, 2, 3):
        s.run(k)
        g = s.last_gains()
        if prev is not None:
            left = g >= 0
            assert np.all(g[left] <= prev[left] + tol) and (g < 0).sum() == (prev < 0).sum() + 1
        prev = g


def test_mixed_recording(runs):
    name = "poly3_67"
    got, sp = runs(name), sc.cases()[name]["special"]
    assert got["status"][sp["three"]] == 1 and got["corners"][sp["three"]] == 3 and sp["three"] not in got["order"]
    assert got["status"][sp["behind"]] == 2 and got["behind"][sp["behind"]] == 1 and sp["behind"] in got["order"]
    assert len(got["order"]) == 66 and np.all(got["I"][sp["three"]] == 0.0)
    a, b = sp["twins"]
    assert np.array_equal(got["I"][a], got["I"][b])
    ka, kb = int(np.where(got["order"] == a)[0][0]), int(np.where(got["order"] == b)[0][0])
    assert ka < kb and got["gain"][kb] < got["gain"][ka]          # exactly equal gains: the lower frame first; the twin then gains strictly less


def test_all_frames_selected_reach_total(runs):
    got, tol = runs("k_equals_n"), sc.tolerances("k_equals_n")
    assert len(got["order"]) == 5 and abs(got["cum"][-1] - got["total"]) <= tol["cum"] + tol["total"]


def test_start_set_is_a_continuation(runs):
    name = "stereo_fov"
    full, tol = runs(name), sc.tolerances(name)
    cont = device_select(sc.cases()[name], k=3, start=[int(full["order"][0])], with_information=False)
    assert np.array_equal(cont["order"], full["order"][1:])
    assert np.abs(cont["gain"] - full["gain"][1:]).max() <= tol["gain"]
    assert np.abs(cont["cum"] - (full["cum"][1:] - full["cum"][0])).max() <= 2 * tol["cum"]


def test_run_argument_errors_and_stale_reads():
    c = sc.cases()["stereo_fov"]
    s = selector_of(c)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.result()                                   # nothing has run
    for k, start, prior in ((0, (), 1e-6), (3, (12,), 1e-6), (3, (-1,), 1e-6), (3, (2, 2), 1e-6), (3, (), 0.0), (3, (), -1.0), (3, (), np.nan), (3, (), np.inf)):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            s.run(k, start, prior)
    want = s.run(4)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.run(0)
    got = s.result()                                 # a refused run left the handle unchanged
    assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["gain"], want["gain"])
    tf, tc, off, pid = sc.flat(c)
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.add_tiles(tf[:1], [2], off[:2], c["points"], pid)          # a camera >= n_cameras
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.add_tiles(tf[:1], tc[:1], off[:2], c["points"][:5], pid)   # a point id >= n_points
    assert np.array_equal(s.result()["order"], want["order"])
    s.add_tiles([12], [0], [0, 4], c["points"], [0, 1, 20, 21])      # a frame without a pose
    for reader in (s.result, s.frames, s.last_gains, lambda: s.frame_information(0)):
        with pytest.raises(lib.VicalibError, match="BAD_ARG"):
            reader()                                 # never stale data
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.run(4)                                     # poses missing
    s.set_poses(np.concatenate([c["poses"], c["poses"][:1]]))
    assert len(s.run(4)["order"]) == 4


def test_timer_leaves_the_result_alone(runs):
    s = selector_of(sc.cases()["stereo_fov"])
    with pytest.raises(lib.VicalibError, match="BAD_ARG"):
        s.time(2)
    s.run(4)
    before = read(s)
    ms = s.time(2)
    assert ms.shape == (3,) and np.all(ms > 0)
    after = read(s)
    assert all(np.array_equal(before[k], after[k]) for k in ("order", "gain", "cum", "I", "last_gains"))


def test_selector_of_a_solved_calibrator():
    """vc_selector_create_for_calibrator on a solved vision-only problem against the standalone handle fed the same cameras, poses and tiles"""
    prob = synth.generate(synth.Config(models=("poly3", "poly3"), n_frames=10, seed=3, pixel_sigma=0.1))
    cal = ViCalibrator(0)
    for c in range(2):
        cal.AddCamera(prob.cam_model[c], prob.cam_K_gt[c], prob.cam_T_ck_gt[c], prob.cfg.width, prob.cfg.height)
    for f in range(len(prob.frame_time)):
        cal.AddFrame(prob.frame_T_wk_gt[f], prob.frame_time[f])
    for (f, c, ids, pix) in prob.tiles:
        cal.AddObservations(f, c, prob.grid_points[ids], pix)
    cal.SetCalibrateImu(False)
    cal.Solve()
    mine = Selector.for_calibrator(cal)
    assert mine.D == 7 + 13 and mine.n_frames == 10      # camera 0 pinned, camera 1 free
    mine.run(5)
    cams = [("poly3",) + cal.GetCamera(c) + (fl,) for c, fl in ((0, lib.CAM_K_FREE), (1, lib.CAM_ROT_FREE | lib.CAM_TRANS_FREE | lib.CAM_K_FREE))]
    case = dict(cameras=cams, poses=cal.GetFrames(), tiles=[(f, c, ids) for (f, c, ids, pix) in prob.tiles], points=prob.grid_points)
    other = selector_of(case)
    other.run(5)
    a, b = read(mine), read(other)
    for key in ("order", "gain", "cum", "I", "scale", "status", "corners", "last_gains"):
        assert np.array_equal(a[key], b[key]), key
    assert a["total"] == b["total"] and len(a["order"]) == 5
    cal.FixCameraIntrinsics(True)
    assert Selector.for_calibrator(cal).D == 6           # extrinsics only


def test_cli_end_to_end(tmp_path):
    """a small vision-only solve with -select_views: both files, ranks contiguous, shares non-decreasing and <= 1; with -holdout_every the held-out
    frames are scored as well"""
    prob = synth.generate(synth.Config(models=("poly3",), n_frames=16, seed=7, pixel_sigma=0.1))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    out = tmp_path / "sel"
    r = subprocess.run([BIN, "-cam", "detections://" + files[0], "-models", "poly3", "-nocalibrate_imu", "-output", str(tmp_path / "cameras.xml"), "-select_views", "6",
                        "-select_dir", str(out), "-holdout_every", "4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = list(csv.DictReader(open(out / "selected_views.csv")))
    assert list(rows[0].keys()) == ["rank", "frame", "gain", "cum", "share"]
    assert [int(x["rank"]) for x in rows] == list(range(1, 7))
    share = np.array([float(x["share"]) for x in rows])
    assert np.all(np.diff(share) >= 0) and np.all(share <= 1.0) and share[0] > 0
    held = [3, 7, 11, 15]
    assert len({int(x["frame"]) for x in rows}) == 6 and not {int(x["frame"]) for x in rows} & set(held)
    frames = list(csv.DictReader(open(out / "select_frames.csv")))
    assert list(frames[0].keys()) == ["frame", "status", "corners", "behind", "first_round_gain"]
    assert [int(x["frame"]) for x in frames] == [f for f in range(16) if f not in held] and all(x["status"] == "0" for x in frames)
    best = max(frames, key=lambda x: float(x["first_round_gain"]))
    assert best["frame"] == rows[0]["frame"] and float(best["first_round_gain"]) == float(rows[0]["gain"])
    hold = list(csv.DictReader(open(out / "select_holdout.csv")))
    assert [int(x["frame"]) for x in hold] == held and sorted(int(x["rank"]) for x in hold) == [1, 2, 3, 4]
    assert all(float(x["first_round_gain"]) > 0 for x in hold)
    assert re.search(r"selected views: 6 of 12 usable frames \(7 shared columns\); .* reach 90 %, .* reach 99 %", r.stdout), r.stdout
    # off unless asked for
    r2 = subprocess.run([BIN, "-cam", "detections://" + files[0], "-models", "poly3", "-nocalibrate_imu", "-output", str(tmp_path / "cameras2.xml")], cwd=str(tmp_path),
                        capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and "selected views" not in r2.stdout
