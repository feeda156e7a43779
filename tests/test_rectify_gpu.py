"""Stereo rectification on the device (vc_rectif*, vicalib_amd/csrc/vc_rectify.hip): the stereo consistency check k_rectify_check against the
numpy reference of tests/rectify_cases.py (the oracle's projection inverted by bisection, Kabsch by SVD; computed once per case), its
determinism and structure, invalid pairs, a wrong baseline, the image pairs and maps of the two sides against the undistorter, and the
command line.  One launch covers frames of 0, 1, 2, 3, 5, 63, 64, 65, 130 and 190 pairs."""
import os
import re
import subprocess

import numpy as np
import pytest

import rectify_cases as rc
import undistort_cases as uc
from vicalib_amd import synth
from vicalib_amd.lib import Rectifier, Undistorter, ViCalibrator

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vicalib_amd", "vicalib")
SMALL = (96, 72)


def rectifier(c, T_ck=None, dst_size=SMALL, dl=rc.DST_LINEAR):
    """(the check reads no image: a small destination keeps the two lookup tables small)"""
    T = c.T_ck if T_ck is None else T_ck
    return Rectifier((c.models[0], c.K[0], rc.SIZE, T[0]), (c.models[1], c.K[1], rc.SIZE, T[1]), dst_size=dst_size, dst_linear=dl)


def run(c, r=None, target=True):
    r = rectifier(c) if r is None else r
    return r.check(c.frame_off, c.px_a, c.px_b, c.target if target else None)


def same_bits(a, b, keys=("pairs", "invalid", "count", "n_invalid", "sum_dv", "sum_dv2", "max_abs_dv", "worst", "mean_z", "rigid_rms")):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


@pytest.mark.parametrize("models", rc.MODEL_PAIRS)
def test_exact_data(models):
    c = rc.check_case(models, 0.0)
    r = rectifier(c)
    out = run(c, r)
    e_dv, e_p, rms = rc.check_exact(c, out, r.get()["R_ds_a"])
    print("%s exact: max |dv| %.3g px, max |P - R_ds_a p_a| %.3g m, max rigid_rms %.3g m" % ("/".join(models), e_dv, e_p, rms))
    rc.check_frame_rows(c, out)
    assert list(out["count"]) == list(rc.FRAME_SIZES)


@pytest.mark.parametrize("models", rc.MODEL_PAIRS)
def test_noisy_data_against_numpy(models):
    c = rc.check_case(models, 0.1)
    r = rectifier(c)
    out = run(c, r)
    e_px, e_m = rc.check_pairs_against_reference(out, *rc.reference("noisy", models))
    rc.check_frame_rows(c, out)
    rms_dv = np.sqrt(out["sum_dv2"][5:] / out["count"][5:])
    print("%s noisy: device - numpy %.3g px, %.3g m; rms dv %.3f - %.3f px, rigid_rms %.3g - %.3g m"
          % ("/".join(models), e_px, e_m, rms_dv.min(), rms_dv.max(), out["rigid_rms"][5:].min(), out["rigid_rms"][5:].max()))
    # two runs give the same bits
    assert same_bits(out, run(c, r))
    # a frame launched alone gives the same bits as in the batch
    for k in (4, 7, 9):
        s = rc.frames_of(c)[k]
        alone = r.check([0, s.stop - s.start], c.px_a[s], c.px_b[s], c.target[s])
        assert np.array_equal(alone["pairs"], out["pairs"][s]) and alone["worst"][0] == out["worst"][k] - s.start
        for key in ("count", "n_invalid", "sum_dv", "sum_dv2", "max_abs_dv", "mean_z", "rigid_rms"):
            assert alone[key][0] == out[key][k], (k, key)
    # without target points: no rigid fit, everything else the same bits
    bare = run(c, r, target=False)
    assert np.isnan(bare["rigid_rms"]).all() and same_bits(out, bare, keys=("pairs", "invalid", "count", "sum_dv", "sum_dv2", "max_abs_dv", "worst", "mean_z"))
    # a check of no frames launches nothing
    assert len(r.check([0], np.zeros((0, 2)), np.zeros((0, 2)))["count"]) == 0


def test_worst_is_the_lowest_index_on_ties():
    c = rc.check_case(("kb4", "poly3"), 0.1)
    r = rectifier(c)
    out = run(c, r)
    k = 8                                                    # the 130-pair frame: three lanes hold the same |dv|
    s = rc.frames_of(c)[k]
    w = int(out["worst"][k])
    a, b = c.px_a.copy(), c.px_b.copy()
    for j in (s.start, s.stop - 1):
        a[j], b[j] = a[w], b[w]
    tied = r.check(c.frame_off, a, b, c.target)
    assert tied["worst"][k] == s.start and tied["max_abs_dv"][k] == out["max_abs_dv"][k]
    assert tied["pairs"][s.start, 0] == tied["pairs"][w, 0] == tied["pairs"][s.stop - 1, 0]


@pytest.mark.parametrize("name", ["beyond", "swapped"])
def test_invalid_pairs(name):
    c = rc.beyond_case() if name == "beyond" else rc.swapped_case()
    out = run(c)
    ref_pairs, ref_bad = rc.reference(name)
    assert np.array_equal(np.nonzero(ref_bad)[0], c.bad)                      # the reference flags the injected pair and no other
    rc.check_pairs_against_reference(out, ref_pairs, ref_bad)                 # ... and so does the device; the bad pair's row is NaN
    assert np.isnan(out["pairs"][c.bad]).all() and out["invalid"][c.bad].all()
    rc.check_frame_rows(c, out)                                               # the sums are those of the valid pairs
    k = int(np.searchsorted(c.frame_off, c.bad[0], side="right") - 1)
    assert c.frame_off[k + 1] - c.frame_off[k] == 65
    assert out["count"][k] == 65 - 1 and out["n_invalid"][k] == 1 and out["n_invalid"].sum() == 1


def test_both_invalid_pairs_in_one_frame():
    """the swapped pair and a pixel beyond the image in the 65-pair frame of one launch: n - 2 valid"""
    c = rc.swapped_case()
    a = c.px_a.copy()
    far = int(c.frame_off[7] + 40)
    a[far] = [1e7, -3e6]                                     # kb4's polynomial never reaches this radius inside theta <= pi
    out = rectifier(c).check(c.frame_off, a, c.px_b, c.target)
    assert out["count"][7] == 65 - 2 and out["n_invalid"][7] == 2 and sorted(np.nonzero(out["invalid"])[0]) == sorted([int(c.bad[0]), far])
    ref = rc.Case(); ref.__dict__.update(c.__dict__); ref.px_a = a
    rc.check_frame_rows(ref, out)


def test_a_wrong_baseline_shows_in_metres_not_in_rows():
    c = rc.check_case(("fov", "fov"), 0.0)
    Tb = c.T_ck[1].copy(); Tb[4:] *= 1.02
    out = run(c, rectifier(c, T_ck=[c.T_ck[0], Tb]))
    full = np.asarray(out["count"]) >= 3
    print("t_bk x 1.02: rigid_rms %.3g - %.3g m, max |dv| %.3g px" % (out["rigid_rms"][full].min(), out["rigid_rms"][full].max(), np.abs(out["pairs"][:, 0]).max()))
    assert out["rigid_rms"][full].min() > 1e-4 and np.abs(out["pairs"][:, 0]).max() < 1e-9


def test_sides_are_undistorters_with_the_rectifying_rotations():
    c = rc.check_case(("kb4", "poly3"), 0.0)
    Ks = [k.copy() for k in c.K]
    for k in Ks:
        k[:4] *= 0.125                                       # 80 x 60 sources
    src = (80, 60)
    r = Rectifier(("kb4", Ks[0], src, c.T_ck[0]), ("poly3", Ks[1], src, c.T_ck[1]), dst_size=(67, 35), alpha=0.3)
    g = r.get()
    Ra, Rb, b = Rectifier.rotations(c.T_ck[0], c.T_ck[1])
    assert np.array_equal(g["R_ds_a"], Ra) and np.array_equal(g["R_ds_b"], Rb) and g["baseline"] == b and g["dst_size"] == (67, 35)
    dl = Rectifier.fit_linear(("kb4", Ks[0], src), Ra, ("poly3", Ks[1], src), Rb, (67, 35), alpha=0.3)
    assert np.array_equal(g["dst_linear"], dl)
    # T_ck_rect = (R_ds R_ck, R_ds t_ck): the same rotation, centres apart by the baseline along x
    (Rra, tra), (Rrb, trb) = rc.pose_Rt(g["T_ck_rect_a"]), rc.pose_Rt(g["T_ck_rect_b"])
    assert np.abs(Rra - Rrb).max() <= 1e-12 and np.abs((trb - tra) - [-b, 0, 0]).max() <= 1e-12
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (3, src[1], src[0]), dtype=np.uint8) for _ in range(2)]
    got = r.pairs(imgs[0], imgs[1])
    for s, (model, R) in enumerate((("kb4", Ra), ("poly3", Rb))):
        side = r.side(s)
        assert np.array_equal(side.linear()[0], dl)
        m, valid = side.map()
        want, z = uc.oracle_map(model, Ks[s], dl, R, src, (67, 35))
        uc.check_map(model, src, m, valid, want, z)
        assert valid.any() and (s == 0 or (~valid).any())      # (kb4's field is wider than anything the pair shares)
        # the same bytes as the side's own remap, and as an undistorter made from the same numbers
        assert np.array_equal(got[s], side.images(imgs[s]))
        assert np.array_equal(got[s], Undistorter(model, Ks[s], src, dl, (67, 35), R).images(imgs[s]))
    rr = rectifier(c)
    with pytest.raises(Exception):
        rr.time(reps=2)                                      # nothing to time before a check
    run(c, rr)
    assert rr.time(reps=2) > 0


def _csv(path):
    rows = [line.strip().split(",") for line in open(path)]
    return rows[0], np.array([[float(x) for x in r] for r in rows[1:]])


def test_cli_rectify_dir(tmp_path):
    prob = synth.generate(synth.Config(models=("fov", "poly3"), n_frames=14, seed=3))
    files, _ = synth.write_dataset(prob, str(tmp_path))
    out, rdir = tmp_path / "cameras.xml", tmp_path / "rect"
    args = ["-cam", "detections://" + ",".join(files), "-models", "fov,poly3", "-nocalibrate_imu", "-output", str(out)]
    r = subprocess.run([BIN] + args + ["-rectify_dir", str(rdir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stderr.splitlines() if x.startswith("I cameras 0,1 rectified")]
    assert len(line) == 1 and "baseline" in line[0] and "rms dv" in line[0] and "worst |dv|" in line[0] and "median rigid_rms_m" in line[0]
    # the XML: two linear cameras with the same intrinsics and rotation, centres apart along the rectified x axis only
    txt = open(rdir / "cameras.xml").read()
    assert txt.count('type="calibu_fu_fv_u0_v0"') == 2
    params = [np.array([float(x) for x in p.split(";")]) for p in re.findall(r"<params>\s*\[(.*?)\]", txt, re.S)]
    T = [np.array([[float(x) for x in row.split(",")] for row in t.split(";")]) for t in re.findall(r"<T_wc>\s*\[(.*?)\]", txt, re.S)]
    assert np.array_equal(params[0], params[1]) and np.abs(T[0][:, :3] - T[1][:, :3]).max() <= 1e-12
    step = T[0][:, :3].T @ (T[1][:, 3] - T[0][:, 3])
    assert abs(step[1]) <= 1e-12 and abs(step[2]) <= 1e-12 and 0.05 < step[0] < 0.07          # the generator's rig: 6 cm
    # the CSV: the Python wrapper's check on the solved cameras over the same matched detections
    solved = re.findall(r"<params>\s*\[(.*?)\]", open(out).read(), re.S)
    K = [np.array([float(x) for x in p.split(";")]) for p in solved]
    Twc = [np.array([[float(x) for x in row.split(",")] for row in t.split(";")]) for t in re.findall(r"<T_wc>\s*\[(.*?)\]", open(out).read(), re.S)]
    T_ck = [rc.pose(M[:, :3].T, -M[:, :3].T @ M[:, 3]) for M in Twc]
    Ra, Rb, _ = Rectifier.rotations(T_ck[0], T_ck[1])
    dl = Rectifier.fit_linear(("fov", K[0], rc.SIZE), Ra, ("poly3", K[1], rc.SIZE), Rb)
    np.testing.assert_allclose(dl, params[0], rtol=1e-9)
    rect = Rectifier(("fov", K[0], rc.SIZE, T_ck[0]), ("poly3", K[1], rc.SIZE, T_ck[1]), dst_linear=params[0])
    tf, tc, off, pw, pc = synth.flatten(prob)
    ids = np.concatenate([t[2] for t in prob.tiles])
    frames, foff, pa, pb = Rectifier.match_tiles(tf, tc, off, ids, 0, 1)
    want = rect.check(foff, pc[pa], pc[pb], pw[pa])
    head, rows = _csv(rdir / "stereo_check.csv")
    assert head == ["frame", "pairs", "invalid", "mean_dv", "rms_dv", "max_abs_dv", "mean_z_m", "rigid_rms_m"]
    assert np.array_equal(rows[:, 0], frames) and np.array_equal(rows[:, 1], want["count"] + want["n_invalid"]) and np.array_equal(rows[:, 2], want["n_invalid"])
    cnt = want["count"]
    cols = [want["sum_dv"] / cnt, np.sqrt(want["sum_dv2"] / cnt), want["max_abs_dv"], want["mean_z"], want["rigid_rms"]]
    for j, col in enumerate(cols):                           # (%.10g in the file; the cameras come through the XML's %.17g and a quaternion)
        np.testing.assert_allclose(rows[:, 3 + j], col, rtol=1e-8, atol=1e-10)
    assert len(rows) == 14 and rows[:, 1].min() > 100 and np.sqrt(want["sum_dv2"].sum() / cnt.sum()) < 1.0 and np.nanmax(want["rigid_rms"]) < 5e-3
    # a bad pair of cameras, or a single camera: an E line, exit status 1, before anything is solved
    for extra, cams in ((["-rectify_cams", "0,0"], files), (["-rectify_cams", "0,2"], files), (["-rectify_cams", "1"], files), ([], files[:1])):
        r = subprocess.run([BIN, "-cam", "detections://" + ",".join(cams), "-models", "fov,poly3", "-nocalibrate_imu", "-output", str(tmp_path / "x.xml"),
                            "-rectify_dir", str(tmp_path / "none")] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and any(x.startswith("E ") and "rectify" in x for x in r.stderr.splitlines()) and not (tmp_path / "none").exists(), r.stderr[-500:]


def test_rectifier_for_cameras_of_a_calibrator():
    c = rc.check_case(("rational6", "poly2"), 0.0)
    cal = ViCalibrator(0)
    for m, K, T in zip(c.models, c.K, c.T_ck):
        cal.AddCamera(m, K, T, *rc.SIZE)
    a = Rectifier.for_cameras(cal, 0, 1, rc.SIZE, dst_size=SMALL, dst_linear=rc.DST_LINEAR)
    assert same_bits(run(c, a), run(c))
    with pytest.raises(Exception):
        Rectifier.for_cameras(cal, 0, 0, rc.SIZE, dst_size=SMALL, dst_linear=rc.DST_LINEAR)
